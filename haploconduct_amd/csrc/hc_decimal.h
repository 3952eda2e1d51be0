// hc_decimal.h — std::to_string of an unsigned / an int on the device: how many characters, and the characters.  Shared by the
// kernels that write text (hc_fno_kernels.hip, hc_graph_text_kernels.hip); no division beyond / 10 and % 10, no libm.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hc {

__device__ __forceinline__ uint32_t digits_u64(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}
__device__ __forceinline__ uint32_t chars_i32(int32_t x) {
    const uint32_t v = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;
    return digits_u64(v) + (x < 0 ? 1u : 0u);
}
__device__ __forceinline__ char* put_u64(char* p, uint64_t v) {
    char tmp[20];
    int n = 0;
    do {
        tmp[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) *p++ = tmp[--n];
    return p;
}
// the same for a value below 2^32 (vertex ids) in 32-bit arithmetic: no 64-bit multiply-high per digit
__device__ __forceinline__ uint32_t digits_u32(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ char* put_u32(char* p, uint32_t v) {
    const uint32_t n = digits_u32(v);
    for (uint32_t k = n; k-- > 0;) {
        p[k] = (char)('0' + v % 10u);
        v /= 10u;
    }
    return p + n;
}
__device__ __forceinline__ char* put_i32(char* p, int32_t x) {  // std::to_string(int)
    if (x < 0) *p++ = '-';
    return put_u64(p, x < 0 ? 0u - (uint32_t)x : (uint32_t)x);
}

}  // namespace hc
