// hc_sr_fastq_kernels.hip — the device side of hc_sr_fastq_write_text (include/hcsr.h): the text of singles.fastq, paired1.fastq,
// paired2.fastq and removed_tip_sequences.fastq (reference src/SRBuilder.cpp:1386-1556) from raw arrays that are on the device.
//
// fq_sizes_kernel: one lane per read and one per tip.  A read's lane writes the characters of its record in each of the three files
//   (0 where it does not belong), a tip's lane those of its one or two records; the '@' lines are counted per wave and added to four
//   counters.  Items and their order: hc_sr_fastq.h.
// fq_bounds_kernel: one lane copies the five file boundaries out of the exclusive sum, next to the record counters, so that one small
//   copy brings all of hc_sr_fastq_counts back.
// fq_write_kernel: one wave per item.  Lane 0 writes '@', the id, the "_1" / "_2" of a paired tip and the newlines with the '+'; the
//   wave copies sequence and quality with wave_copy (hc_wave_copy.h: 16-byte stores on 16-byte boundaries of the text whatever the id's
//   digit count made of the record's start, head and tail bytewise).  No atomics in the write pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_decimal.h"
#include "hc_sr_fastq.h"
#include "hc_wave_copy.h"

namespace hc {
namespace fastq {
namespace {

constexpr int kBlock = 256;

// "@" id suffix "\n" SEQ "\n+\n" QUAL "\n": 6 characters beside the id, its suffix and the bytes twice
__device__ __forceinline__ uint64_t record_chars(uint32_t id_chars, uint32_t len) { return (uint64_t)id_chars + 2ull * len + 6ull; }

__device__ __forceinline__ uint32_t seq_len(const Store& s, uint32_t q) { return (uint32_t)(s.off[q + 1] - s.off[q]); }

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kBlock) void fq_sizes_kernel(Store cur, Tips tips, uint64_t* __restrict__ sizes, unsigned long long* __restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x, n = cur.n_reads;
    uint32_t rec[4] = {0, 0, 0, 0};  // '@' lines of this lane per file
    if (i < n) {
        const uint32_t r = (uint32_t)i, q = cur.first[r], d = digits_u32(r);
        const bool paired = cur.first[r + 1] - q == 2;
        sizes[i] = paired ? 0ull : record_chars(d, seq_len(cur, q));
        sizes[n + i] = paired ? record_chars(d, seq_len(cur, q)) : 0ull;
        sizes[2 * n + i] = paired ? record_chars(d, seq_len(cur, q + 1)) : 0ull;
        rec[0] = !paired;
        rec[1] = rec[2] = paired;
    } else if (i - n < tips.n) {
        const uint64_t k = i - n;
        const uint32_t r = tips.reads[k], q = tips.store.first[r], d = digits_u32((uint32_t)k);
        const bool paired = tips.store.first[r + 1] - q == 2;
        sizes[3 * n + k] = paired ? record_chars(d + 2, seq_len(tips.store, q)) + record_chars(d + 2, seq_len(tips.store, q + 1))
                                  : record_chars(d, seq_len(tips.store, q));
        rec[3] = paired ? 2u : 1u;
    } else if (i - n == tips.n) {
        sizes[3 * n + tips.n] = 0;
    }
    for (int f = 0; f < 4; f++) {
        const uint32_t c = wave_sum(rec[f]);  // (every lane of the wave is here)
        if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&counters[f], (unsigned long long)c);
    }
}

__global__ void fq_bounds_kernel(uint32_t n_reads, uint64_t n_tips, const uint64_t* __restrict__ pos, unsigned long long* __restrict__ counters) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t n = n_reads;
    counters[4] = pos[0];
    counters[5] = pos[n];
    counters[6] = pos[2 * n];
    counters[7] = pos[3 * n];
    counters[8] = pos[3 * n + n_tips];
}

// one record at p: lane 0 the frame, the wave the bytes.  suffix: 0, or '1' / '2' for "_1" / "_2".  Returns the record's end.
__device__ inline char* put_record(char* p, uint32_t id, char suffix, const Store& s, uint32_t q, uint32_t lane) {
    const uint64_t off = s.off[q];
    const uint32_t len = (uint32_t)(s.off[q + 1] - off), head = 2u + digits_u32(id) + (suffix ? 2u : 0u);
    if (lane == 0) {
        p[0] = '@';
        char* e = put_u32(p + 1, id);
        if (suffix) {
            e[0] = '_';
            e[1] = suffix;
            e += 2;
        }
        e[0] = '\n';
        char* m = p + head + len;
        m[0] = '\n';
        m[1] = '+';
        m[2] = '\n';
        m[3 + len] = '\n';
    }
    wave_copy<false, false>((uint8_t*)p + head, s.bases + off, len, lane);
    wave_copy<false, false>((uint8_t*)p + head + len + 3u, s.quals + off, len, lane);
    return p + head + 2ull * len + 4u;
}

__global__ __launch_bounds__(kBlock) void fq_write_kernel(Store cur, Tips tips, const uint64_t* __restrict__ pos, char* __restrict__ text) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n = cur.n_reads, n_it = 3 * n + tips.n;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock >> 6);
    for (uint64_t i = (uint64_t)blockIdx.x * (kBlock >> 6) + (threadIdx.x >> 6); i < n_it; i += n_waves) {  // (i is wave-uniform)
        if (i < 3 * n) {
            const uint32_t f = (uint32_t)(i >= n) + (uint32_t)(i >= 2 * n), r = (uint32_t)(i - (uint64_t)f * n), q = cur.first[r];
            const bool paired = cur.first[r + 1] - q == 2;
            if (paired != (f != 0)) continue;  // the read is not in this file
            put_record(text + pos[i], r, 0, cur, q + (f == 2), lane);
        } else {
            const uint64_t k = i - 3 * n;
            const uint32_t r = tips.reads[k], q = tips.store.first[r];
            char* p = text + pos[i];
            if (tips.store.first[r + 1] - q == 2) {  // :1394-1403
                p = put_record(p, (uint32_t)k, '1', tips.store, q, lane);
                put_record(p, (uint32_t)k, '2', tips.store, q + 1, lane);
            } else {  // :1405-1410
                put_record(p, (uint32_t)k, 0, tips.store, q, lane);
            }
        }
    }
}

inline uint32_t lane_grid(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }  // (n >= 1, below 2^33)
inline uint32_t wave_grid(uint64_t n_waves) {  // workgroups of four waves, at most 2^16 of them (the kernel strides)
    const uint64_t w = (n_waves + 3) / 4;
    return (uint32_t)(w < 1 ? 1 : (w > 65536 ? 65536 : w));
}

}  // namespace

hipError_t launch_sizes(Store cur, Tips tips, uint64_t* sizes, unsigned long long* counters, hipStream_t stream) {
    hipLaunchKernelGGL(fq_sizes_kernel, dim3(lane_grid((uint64_t)cur.n_reads + tips.n + 1)), dim3(kBlock), 0, stream, cur, tips, sizes, counters);
    return hipGetLastError();
}

hipError_t launch_bounds(uint32_t n_reads, uint64_t n_tips, const uint64_t* pos, unsigned long long* counters, hipStream_t stream) {
    hipLaunchKernelGGL(fq_bounds_kernel, dim3(1), dim3(64), 0, stream, n_reads, n_tips, pos, counters);
    return hipGetLastError();
}

hipError_t launch_write(Store cur, Tips tips, const uint64_t* pos, char* text, hipStream_t stream) {
    hipLaunchKernelGGL(fq_write_kernel, dim3(wave_grid(n_items(cur.n_reads, tips.n))), dim3(kBlock), 0, stream, cur, tips, pos, text);
    return hipGetLastError();
}

}  // namespace fastq
}  // namespace hc
