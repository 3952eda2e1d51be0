// hc_wave_copy.h — one wave copies a run of bytes to a destination of any alignment, forwards or back to front, plain or through
// build_rev_comp's mapping (hc_sr_next.h: sr_next_complement).  Shared by the kernels that move read bytes: the next store's
// gather (hc_sr_next_kernels.hip) and the GFA segment lines (hc_graph_text_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr_next.h"

namespace hc {

// d[i] = s[i], or with REV s[len - 1 - i] (COMP: through build_rev_comp's mapping), for i in [0, len), by one wave
template <bool REV, bool COMP>
__device__ inline void wave_copy(uint8_t* d, const uint8_t* s, uint32_t len, uint32_t lane) {
    auto one = [&](uint32_t i) {
        const uint8_t b = s[REV ? len - 1u - i : i];
        d[i] = COMP ? sr_next_complement(b) : b;
    };
    uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
    if (head > len) head = len;
    if (lane < head) one(lane);
    const uint32_t nvec = (len - head) >> 4;
    for (uint32_t v = lane; v < nvec; v += 64) {
        const uint32_t i0 = head + (v << 4);  // i0 + 16 <= len
        uint4 w;  // (the source starts anywhere)
        __builtin_memcpy(&w, REV ? s + (len - i0 - 16u) : s + i0, 16);
        if (REV) w = make_uint4(__builtin_bswap32(w.w), __builtin_bswap32(w.z), __builtin_bswap32(w.y), __builtin_bswap32(w.x));
        if (COMP) {
            uint32_t* p = (uint32_t*)&w;
            for (int k = 0; k < 4; k++) {
                const uint32_t x = p[k];
                p[k] = (uint32_t)sr_next_complement((uint8_t)x) | (uint32_t)sr_next_complement((uint8_t)(x >> 8)) << 8 |
                       (uint32_t)sr_next_complement((uint8_t)(x >> 16)) << 16 | (uint32_t)sr_next_complement((uint8_t)(x >> 24)) << 24;
            }
        }
        *(uint4*)(d + i0) = w;
    }
    const uint32_t t0 = head + (nvec << 4);
    if (lane < len - t0) one(t0 + lane);
}

}  // namespace hc
