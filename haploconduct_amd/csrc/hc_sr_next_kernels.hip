// hc_sr_next_kernels.hip — the device side of hc_sr_set_next_reads (include/hcsr.h): the next iteration's raw read arrays from the
// kept consensus bytes, the call's extra bytes and the current raw arrays, without a copy through the host.
//
// sr_next_check_kernel: one wave per entry.  The wave resolves the entry (hc_sr_next.h: the range checks; nothing is read for a bad one),
//   counts the N of its mates — 16-byte loads from the first 16-byte boundary on, a packed-byte compare and a popcount per word, bytes
//   before and behind, a butterfly over the wave — and applies the reference's tests in the reference's order.  It leaves the status and
//   what the two exclusive sums turn into the survivor's rank, first sequence and first byte.
// sr_next_gather_kernel: one wave per surviving entry, mate after mate, 64 x 16 bytes a step: stores on 16-byte boundaries of the new
//   arrays, loads wherever the source starts.  A reverse trivial is written back to front — the 16 bytes of a step reversed in registers,
//   the bases through build_rev_comp's mapping —, a reverse pair has its mates swapped by the resolver.
// sr_next_hist_kernel: byte histograms of the new bases and qualities for hc_set_reads' planning.  Every wave counts into LDS counters of
//   its own and the workgroup folds what is not zero into the 2 x 256 global counters at its end: a few hundred global atomics a
//   workgroup instead of one per byte on a handful of addresses.
// sr_patch_kernel: hc_sr_consensus with keeping on — the columns host threads finished, scattered into the kept bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hc_sr_next.h"
#include "hc_wave_copy.h"

namespace hc {
namespace {

// how many of the four bytes of w are 'N': the zero bytes of w ^ "NNNN", exactly (no carry crosses a byte)
__device__ inline uint32_t count_n_word(uint32_t w) {
    const uint32_t x = w ^ 0x4E4E4E4Eu;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return __popc(~(t | x | 0x7F7F7F7Fu));
}

// this lane's share of the N in p[0, len)
__device__ inline uint32_t lane_count_n(const uint8_t* p, uint32_t len, uint32_t lane) {
    uint32_t head = (uint32_t)((16u - ((uintptr_t)p & 15u)) & 15u);
    if (head > len) head = len;
    uint32_t c = (lane < head && p[lane] == 'N') ? 1u : 0u;
    const uint8_t* a = p + head;  // 16-byte aligned
    const uint32_t rest = len - head, nvec = rest >> 4, tail = rest & 15u;
    for (uint32_t v = lane; v < nvec; v += 64) {
        const uint4 w = ((const uint4*)a)[v];
        c += count_n_word(w.x) + count_n_word(w.y) + count_n_word(w.z) + count_n_word(w.w);
    }
    if (lane < tail && a[(nvec << 4) + lane] == 'N') c++;
    return c;
}

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void sr_next_check_kernel(const hc_sr_next_entry* __restrict__ entries, uint64_t n, SrNextSources S, SrNextBytes B,
                                                            uint32_t keep_singletons, uint32_t* __restrict__ status, uint64_t* __restrict__ cnt,
                                                            uint64_t* __restrict__ bytes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    if (wave == 0 && lane == 0) cnt[n] = bytes[n] = 0;
    for (uint64_t i = wave; i < n; i += n_waves) {
        const hc_sr_next_entry e = entries[i];
        SrNextResolved R;
        uint32_t st = HC_SR_NEXT_BAD_ENTRY;
        uint64_t len = 0;
        if (sr_next_resolve(e, S, R)) {  // (wave-uniform)
            uint32_t c = 0;
            for (uint32_t k = 0; k < R.n_mates; k++) {
                c += lane_count_n(B.seq[R.m[k].src] + R.m[k].off, R.m[k].len, lane);
                len += R.m[k].len;
            }
            st = sr_next_status(e.kind, R, wave_sum(c), keep_singletons);
        }
        if (lane == 0) {
            const bool kept = st == HC_SR_NEXT_KEPT;
            status[i] = st;
            cnt[i] = kept ? (1ull | (uint64_t)R.n_mates << 32) : 0ull;
            bytes[i] = kept ? len : 0ull;
        }
    }
}

// (wave_copy: hc_wave_copy.h)

__global__ __launch_bounds__(256) void sr_next_gather_kernel(const hc_sr_next_entry* __restrict__ entries, uint64_t n, SrNextSources S, SrNextBytes B,
                                                             const uint32_t* __restrict__ status, const uint64_t* __restrict__ cnt_off,
                                                             const uint64_t* __restrict__ byte_off, uint8_t* __restrict__ out_bases,
                                                             uint8_t* __restrict__ out_quals, uint64_t* __restrict__ out_off,
                                                             uint32_t* __restrict__ out_first) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    if (wave == 0 && lane == 0) {  // the closing entries: n_seq and the byte total
        out_first[(uint32_t)cnt_off[n]] = (uint32_t)(cnt_off[n] >> 32);
        out_off[cnt_off[n] >> 32] = byte_off[n];
    }
    for (uint64_t i = wave; i < n; i += n_waves) {
        if (status[i] != HC_SR_NEXT_KEPT) continue;
        SrNextResolved R;
        if (!sr_next_resolve(entries[i], S, R)) continue;  // (kept: it resolved before)
        const uint32_t rank = (uint32_t)cnt_off[i], sidx = (uint32_t)(cnt_off[i] >> 32);
        uint64_t at = byte_off[i];
        if (lane == 0) out_first[rank] = sidx;
        for (uint32_t k = 0; k < R.n_mates; k++) {
            const SrNextMate m = R.m[k];
            if (lane == 0) out_off[sidx + k] = at;
            const uint8_t *sb = B.seq[m.src] + m.off, *sq = B.qual[m.src] + m.off;
            if (R.rev) {
                wave_copy<true, true>(out_bases + at, sb, m.len, lane);
                wave_copy<true, false>(out_quals + at, sq, m.len, lane);
            } else {
                wave_copy<false, false>(out_bases + at, sb, m.len, lane);
                wave_copy<false, false>(out_quals + at, sq, m.len, lane);
            }
            at += m.len;
        }
    }
}

__global__ __launch_bounds__(256) void sr_next_hist_kernel(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, uint64_t total,
                                                           unsigned long long* __restrict__ hist) {
    __shared__ uint32_t h[4][512];  // per wave: [0, 256) qualities, [256, 512) bases
    for (uint32_t i = threadIdx.x; i < 4 * 512; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    uint32_t* mine = h[threadIdx.x >> 6];
    const uint64_t nvec = total >> 4, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {  // (both arrays start on 16-byte boundaries)
        const uint4 q = ((const uint4*)quals)[v], b = ((const uint4*)bases)[v];
        const uint32_t qw[4] = {q.x, q.y, q.z, q.w}, bw[4] = {b.x, b.y, b.z, b.w};
        for (int k = 0; k < 4; k++)
            for (int j = 0; j < 32; j += 8) {
                atomicAdd(&mine[(qw[k] >> j) & 255u], 1u);
                atomicAdd(&mine[256u + ((bw[k] >> j) & 255u)], 1u);
            }
    }
    if (blockIdx.x == 0 && threadIdx.x < (total & 15u)) {  // the bytes behind the last whole vector
        const uint64_t i = (nvec << 4) + threadIdx.x;
        atomicAdd(&mine[quals[i]], 1u);
        atomicAdd(&mine[256u + bases[i]], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 512; i += 256) {
        const unsigned long long s = (unsigned long long)h[0][i] + h[1][i] + h[2][i] + h[3][i];
        if (s) atomicAdd(&hist[i], s);
    }
}

__global__ __launch_bounds__(256) void sr_patch_kernel(const SrPatch* __restrict__ patches, uint64_t n, uint64_t total, uint8_t* __restrict__ seq,
                                                       uint8_t* __restrict__ qual) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SrPatch p = patches[i];
    if (p.off >= total) return;  // (~0: a column that came back NaN)
    seq[p.off] = p.base;
    qual[p.off] = p.qual;
}

inline uint32_t wave_grid(uint64_t n) {  // one wave per item in workgroups of four, at most 2^16 workgroups (the kernels stride)
    const uint64_t g = (n + 3) / 4;
    return (uint32_t)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

hipError_t sr_next_launch_check(const hc_sr_next_entry* entries, uint64_t n, SrNextSources S, SrNextBytes B, uint32_t keep_singletons,
                                uint32_t* status, uint64_t* cnt, uint64_t* bytes, hipStream_t stream) {
    hipLaunchKernelGGL(sr_next_check_kernel, dim3(wave_grid(n)), dim3(256), 0, stream, entries, n, S, B, keep_singletons, status, cnt, bytes);
    return hipGetLastError();
}

hipError_t sr_next_launch_gather(const hc_sr_next_entry* entries, uint64_t n, SrNextSources S, SrNextBytes B, const uint32_t* status,
                                 const uint64_t* cnt_off, const uint64_t* byte_off, uint8_t* out_bases, uint8_t* out_quals, uint64_t* out_off,
                                 uint32_t* out_first, hipStream_t stream) {
    hipLaunchKernelGGL(sr_next_gather_kernel, dim3(wave_grid(n)), dim3(256), 0, stream, entries, n, S, B, status, cnt_off, byte_off, out_bases,
                       out_quals, out_off, out_first);
    return hipGetLastError();
}

hipError_t sr_next_launch_hist(const uint8_t* bases, const uint8_t* quals, uint64_t total, uint32_t n_cu, unsigned long long* hist,
                               hipStream_t stream) {
    const uint64_t want = ((total >> 4) + 255) / 256;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)n_cu * 8));
    hipLaunchKernelGGL(sr_next_hist_kernel, dim3(grid), dim3(256), 0, stream, bases, quals, total, hist);
    return hipGetLastError();
}

hipError_t sr_launch_patch(const SrPatch* patches, uint64_t n, uint64_t total, uint8_t* seq, uint8_t* qual, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sr_patch_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, patches, n, total, seq, qual);
    return hipGetLastError();
}

}  // namespace hc
