// hc_sr_self_kernels.hip — SRBuilder::merge_self_overlap (reference src/SRBuilder.cpp:872-955) for a batch of pairs on the device
// (include/hcsr.h: hc_sr_merge_self_overlaps).
//
// sr_self_scan_kernel: one workgroup per pair, one lane per offset.  The offsets are taken in descending chunks of as many as the
// workgroup has lanes (the reference's order: smallest overlap first, :879-882); a lane adds the log p terms of its offset in position
// order in fp64 — the sum is then overlap_score's (src/EdgeCalculator.cpp:103-137), bit for bit — from a host-built table, multiplies by
// the host-built 1.0 / n and compares with the x-space image of min_score.  After a chunk the workgroup takes the largest offset that
// is a hit or lies in the guard band and stops there (the reference's early exit).  Both mates sit in LDS as (quality row << 3 | base
// code) symbols: at step i every lane reads the same symbol of mate 2 and consecutive symbols of mate 1, nothing comes from device
// memory inside the loop.  Mates of up to kSelfCap symbols are staged once per pair; longer ones go through LDS in windows of
// kSelfWindow positions per chunk, which a lane walks in order, so the sum's order does not change.
// The log table sits in LDS when it fits beside the mates (LDS_LUT) and is read from device memory otherwise.
//
// sr_self_merge_kernel: one lane per output column of the merged pairs: consensus() of {mate 1 at 0, mate 2 at p} (:890-903), the
// quality from the host-built table of one- and two-member columns, the base from the exact sums by comparison (hc_sr_column.h).
// No transcendental function runs on the device.
//
// hc_sr_merge_self_overlaps_kept, whose mates are the consensus bytes the context keeps on the device, has two kernels more.
// sr_self_check_kernel: one wave per pair, what the host-input call's host loop does (the tests of host/SrSelfCheck.h and the batch's
//   quality values).  The range test comes first, is wave-uniform, and nothing is read for a pair it refuses.  Each mate is read in
//   16-byte loads from the 16-byte boundary at or before its first byte on; the bytes of a load that lie outside the mate are masked,
//   so the buffers hold kSelfPad bytes behind the last one.  Validity is decided on packed bytes, four to a word.  A lane keeps the
//   quality bytes it saw as a 128-bit mask; the wave ORs the lanes' masks, adds them to its own only when the pair is valid (as the
//   host does), and at its end the workgroup folds its waves' masks and counters in LDS into a handful of vector atomics.
// sr_self_copy_kernel: one wave per record, 16 bytes a lane and step.  It packs the mates of the pairs the host decides into a staging
//   block, and later writes those pairs' merged reads, uploaded packed, behind the kept bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr_column.h"
#include "hc_sr_self.h"
#include "host/SrSelfCheck.h"

namespace hc {
namespace {

// (row << 3 | code) of a checked symbol (the pairs are checked before the launch: code_or_n); an N takes row K, the all-zero row of the table
__device__ inline uint16_t self_sym(uint8_t base, uint8_t q, const uint8_t* qmap_s, uint32_t K) {
    const uint32_t code = code_or_n(base);
    return (uint16_t)(((code == kCodeN ? K : (uint32_t)qmap_s[q]) << 3) | code);
}

// one position: the term of (a, b) joins the lane's sum
__device__ inline void self_step(uint32_t a, uint32_t b, const double* lut, uint32_t tri, double& S, uint32_t& n) {
    const uint32_t qa = a >> 3, qb = b >> 3;
    const uint32_t hi = qa > qb ? qa : qb, lo = qa > qb ? qb : qa;
    const uint32_t m = ((a ^ b) & 7u) ? 1u : 0u;  // plane 1: the bases differ (an N: row K holds 0.0 in both planes)
    S += lut[m * tri + hi * (hi + 1u) / 2u + lo];
    n += ((a & 7u) < kCodeN && (b & 7u) < kCodeN) ? 1u : 0u;
}

template <bool LDS_LUT>
__global__ __launch_bounds__(256) void sr_self_scan_kernel(const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual,
                                                           const hc_sr_pair* __restrict__ pairs, const uint32_t* __restrict__ skip, uint64_t n_pairs,
                                                           const uint8_t* __restrict__ qmap, const double* __restrict__ lut_g,
                                                           const double* __restrict__ inv_n, SrSelfParams prm, SrSelfScan* __restrict__ out) {
    extern __shared__ double self_smem[];  // [the table, LDS_LUT][mate 1: kSelfCap symbols][mate 2: kSelfCap symbols]
    __shared__ uint8_t qmap_s[256];
    __shared__ int best;
    uint16_t* s1 = (uint16_t*)(self_smem + (LDS_LUT ? prm.lut_doubles : 0u));
    uint16_t* s2 = s1 + kSelfCap;
    const uint32_t tid = threadIdx.x, chunk = blockDim.x;
    if (LDS_LUT)
        for (uint32_t i = tid; i < prm.lut_doubles; i += chunk) self_smem[i] = lut_g[i];
    for (uint32_t i = tid; i < 256; i += chunk) qmap_s[i] = qmap[i];
    const double* lut = LDS_LUT ? (const double*)self_smem : lut_g;
    const uint32_t tri = lut_tri(prm.K + 2u);
    const double ninf = -__builtin_inf();
    for (uint64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        __syncthreads();  // the table and qmap are in place; the last pair's symbols are no longer read
        if (skip[pi]) continue;
        const hc_sr_pair P = pairs[pi];
        const uint8_t *b1 = seq + P.off1, *q1 = qual + P.off1, *b2 = seq + P.off2, *q2 = qual + P.off2;
        const uint32_t len1 = P.len1, len2 = P.len2;
        const bool too_short = len1 < prm.min_read_len || len2 < prm.min_read_len;  // :82-84: every offset scores 0
        const bool resident = len1 <= kSelfCap && len2 <= kSelfCap;
        if (resident) {
            for (uint32_t i = tid; i < len1; i += chunk) s1[i] = self_sym(b1[i], q1[i], qmap_s, prm.K);
            for (uint32_t i = tid; i < len2; i += chunk) s2[i] = self_sym(b2[i], q2[i], qmap_s, prm.K);
        }
        bool found = false;
        const int64_t first = len1 > prm.min_overlap ? (int64_t)len1 - prm.min_overlap : 0;
        for (int64_t p_hi = first; p_hi >= 1; p_hi -= chunk) {
            const int64_t p_lo = p_hi - chunk + 1 > 1 ? p_hi - chunk + 1 : 1;
            if (tid == 0) best = 0;
            const int64_t p = p_hi - tid;
            const bool active = p >= p_lo;
            // (p = len1 when min_overlap is 0: overlap_score returns 0 there, :76-79)
            const uint32_t Lp = (active && !too_short && p < (int64_t)len1) ? min(len1 - (uint32_t)p, len2) : 0u;
            double S = 0.0;
            uint32_t n = 0;
            if (resident) {
                __syncthreads();  // the symbols are staged
                const uint16_t* a = s1 + (active ? p : 0);  // an idle lane (Lp = 0) forms no pointer before the buffer
                for (uint32_t i = 0; i < Lp; i++) self_step(a[i], s2[i], lut, tri, S, n);
            } else {
                const uint32_t Lmax = (too_short || p_lo >= (int64_t)len1) ? 0u : min(len1 - (uint32_t)p_lo, len2);  // the chunk's longest overlap
                for (uint32_t i0 = 0; i0 < Lmax; i0 += kSelfWindow) {
                    __syncthreads();  // the last window is no longer read
                    const uint32_t n2 = min(kSelfWindow, len2 - i0), at1 = i0 + (uint32_t)p_lo, n1 = min(kSelfWindow + chunk - 1u, len1 - at1);
                    for (uint32_t j = tid; j < n2; j += chunk) s2[j] = self_sym(b2[i0 + j], q2[i0 + j], qmap_s, prm.K);
                    for (uint32_t j = tid; j < n1; j += chunk) s1[j] = self_sym(b1[at1 + j], q1[at1 + j], qmap_s, prm.K);
                    __syncthreads();
                    const uint32_t end = min(i0 + kSelfWindow, Lp);
                    const uint16_t* a = s1 + (active ? (uint32_t)(p - p_lo) : 0u);
                    for (uint32_t i = i0; i < end; i++) self_step(a[i - i0], s2[i - i0], lut, tri, S, n);
                }
            }
            __syncthreads();  // best = 0 is written
            // x = (1.0 / total_len) * total_score (:137); -inf where overlap_score returns 0: no counted position, or a term below --mismatch (+inf)
            double x = ninf;
            if (n > 0 && S < __builtin_inf() && n < prm.inv_len) x = inv_n[n] * S;
            const bool hit = active && (prm.always || x > prm.band.hi);
            const bool amb = active && !hit && x > prm.band.lo;
            if (hit || amb) atomicMax(&best, (int)p);
            __syncthreads();
            const int b = best;
            if (b > 0) {
                if (active && p == (int64_t)b) {
                    SrSelfScan r;
                    r.p = b;
                    r.kind = hit ? kSelfHit : kSelfBand;
                    r.x = x;
                    out[pi] = r;
                }
                found = true;
                break;
            }
            __syncthreads();  // everybody has read `best` before the next chunk clears it
        }
        if (!found && tid == 0) {
            SrSelfScan r;
            r.p = -1;
            r.kind = kSelfNone;
            r.x = ninf;
            out[pi] = r;
        }
    }
}

__global__ __launch_bounds__(256) void sr_self_merge_kernel(const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual,
                                                            const hc_sr_pair* __restrict__ pairs, uint64_t n_pairs, const int32_t* __restrict__ mpos,
                                                            const uint64_t* __restrict__ off, uint64_t total, const double* __restrict__ terms,
                                                            const uint8_t* __restrict__ table, uint8_t* __restrict__ out_seq,
                                                            uint8_t* __restrict__ out_qual) {
    __shared__ SrTerms T;
    T.load(terms);
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    // the pair that owns column g: the last i with off[i] <= g (pairs without columns share their successor's offset)
    uint64_t lo = 0, hi = n_pairs;  // off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int32_t p = mpos[lo];
    if (p < 0) return;
    const hc_sr_pair P = pairs[lo];
    const uint32_t c = (uint32_t)(g - off[lo]);
    SrColumn col;
    for (uint32_t k = 0; k < 2; k++) {  // the members in list order: mate 1 at 0, mate 2 at p
        const bool in = k == 0 ? c < P.len1 : c >= (uint32_t)p;
        if (!in) continue;
        const uint64_t at = k == 0 ? P.off1 + c : P.off2 + (c - (uint32_t)p);
        const uint32_t code = code_or_n(seq[at]);
        const uint32_t q = code == kCodeN ? 0u : ((uint32_t)qual[at] - 33u) & 127u;
        col.add(code, q, q, T);  // (the terms of this call are indexed by q itself)
    }
    uint32_t entry = sr::kEntryN;
    if (col.cnt == 1) entry = col.entry1(table);
    else if (col.cnt == 2) entry = col.entry2(table);
    sr_put(entry, col.nuc(col.max_sum()), out_seq[g], out_qual[g]);
}

// This lane's share of the mate [off, off + len) of seq / qual (both 16-byte aligned, readable up to the 16-byte boundary behind the mate):
// bad |= a refused symbol; q_lo / q_hi |= the quality bytes seen, bit (byte & 127)
__device__ inline void lane_check_mate(const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, uint64_t off, uint32_t len, uint32_t lane,
                                       uint32_t& bad, uint64_t& q_lo, uint64_t& q_hi) {
    const uint64_t v0 = off >> 4, v1 = (off + len + 15u) >> 4;  // the 16-byte vectors [v0, v1) cover the mate
    const uint4* sv = (const uint4*)seq;
    const uint4* qv = (const uint4*)qual;
    for (uint64_t v = v0 + lane; v < v1; v += 64) {
        const uint4 b = sv[v], q = qv[v];
        const uint32_t bw[4] = {b.x, b.y, b.z, b.w}, qw[4] = {q.x, q.y, q.z, q.w};
        const int64_t lo = (int64_t)off - (int64_t)(v << 4), hi = (int64_t)(off + len) - (int64_t)(v << 4);  // the mate's bytes of this vector: [lo, hi)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t in = srself::bytes_between(lo - 4 * k, hi - 4 * k);
            bad |= srself::bytes_bad(bw[k], qw[k]) & in;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t qb = (qw[k] >> (8 * j)) & 127u;
                const uint64_t bit = ((in >> (8 * j + 7)) & 1u) ? 1ull << (qb & 63u) : 0ull;
                q_lo |= (qb & 64u) ? 0ull : bit;
                q_hi |= (qb & 64u) ? bit : 0ull;
            }
        }
    }
}

__device__ inline uint32_t wave_or(uint32_t v) {
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void sr_self_check_kernel(const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, uint64_t n_bytes,
                                                            const hc_sr_pair* __restrict__ pairs, uint64_t n_pairs, uint32_t min_overlap,
                                                            uint32_t* __restrict__ status, SrSelfCheckCounters* __restrict__ counters) {
    __shared__ uint32_t w_mask[4][4], w_max_len[4], w_max_first[4];
    __shared__ unsigned long long w_sum_first[4], w_valid[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    // the wave's share over its valid pairs (the same in every lane)
    uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0, max_len = 0, max_first = 0;
    unsigned long long sum_first = 0, n_valid = 0;
    for (uint64_t i = wave; i < n_pairs; i += n_waves) {
        const hc_sr_pair P = pairs[i];
        uint32_t st = HC_SR_SELF_BAD_PAIR;
        if (srself::pair_in_range(n_bytes, P)) {  // (wave-uniform)
            uint32_t bad = 0;
            uint64_t q_lo = 0, q_hi = 0;
            lane_check_mate(seq, qual, P.off1, P.len1, lane, bad, q_lo, q_hi);
            lane_check_mate(seq, qual, P.off2, P.len2, lane, bad, q_lo, q_hi);
            if (wave_or(bad)) {
                st = HC_SR_SELF_BAD_SYMBOL;
            } else {
                st = HC_SR_SELF_NONE;
                m0 |= wave_or((uint32_t)q_lo);
                m1 |= wave_or((uint32_t)(q_lo >> 32));
                m2 |= wave_or((uint32_t)q_hi);
                m3 |= wave_or((uint32_t)(q_hi >> 32));
                const uint32_t f = srself::first_offset(P.len1, min_overlap);
                max_len = max(max_len, max(P.len1, P.len2));
                max_first = max(max_first, f);
                sum_first += f;
                n_valid++;
            }
        }
        if (lane == 0) status[i] = st;
    }
    if (lane == 0) {
        w_mask[wv][0] = m0;
        w_mask[wv][1] = m1;
        w_mask[wv][2] = m2;
        w_mask[wv][3] = m3;
        w_max_len[wv] = max_len;
        w_max_first[wv] = max_first;
        w_sum_first[wv] = sum_first;
        w_valid[wv] = n_valid;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 4) {
        const uint32_t m = w_mask[0][t] | w_mask[1][t] | w_mask[2][t] | w_mask[3][t];
        if (m) atomicOr(&counters->qmask[t], m);
    } else if (t == 4) {
        const unsigned long long v = w_valid[0] + w_valid[1] + w_valid[2] + w_valid[3];
        if (v) {
            atomicAdd((unsigned long long*)&counters->n_valid, v);
            atomicAdd((unsigned long long*)&counters->sum_first, w_sum_first[0] + w_sum_first[1] + w_sum_first[2] + w_sum_first[3]);
            atomicMax(&counters->max_len, max(max(w_max_len[0], w_max_len[1]), max(w_max_len[2], w_max_len[3])));
            atomicMax(&counters->max_first, max(max(w_max_first[0], w_max_first[1]), max(w_max_first[2], w_max_first[3])));
        }
    }
}

// d[0, len) = s[0, len) by one wave: stores on 16-byte boundaries of d, loads wherever s starts
__device__ inline void wave_copy_bytes(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, uint32_t len, uint32_t lane) {
    uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
    if (head > len) head = len;
    if (lane < head) d[lane] = s[lane];
    const uint32_t nvec = (len - head) >> 4;
    for (uint32_t v = lane; v < nvec; v += 64) {
        const uint32_t i0 = head + (v << 4);  // i0 + 16 <= len
        uint4 w;
        __builtin_memcpy(&w, s + i0, 16);
        *(uint4*)(d + i0) = w;
    }
    const uint32_t t0 = head + (nvec << 4);
    if (lane < len - t0) d[t0 + lane] = s[t0 + lane];
}

__global__ __launch_bounds__(256) void sr_self_copy_kernel(const SrSelfSeg* __restrict__ segs, uint64_t n, const uint8_t* __restrict__ src_seq,
                                                           const uint8_t* __restrict__ src_qual, uint8_t* __restrict__ dst_seq,
                                                           uint8_t* __restrict__ dst_qual) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < n; i += n_waves) {
        const SrSelfSeg g = segs[i];
        wave_copy_bytes(dst_seq + g.dst, src_seq + g.src1, g.len1, lane);
        wave_copy_bytes(dst_qual + g.dst, src_qual + g.src1, g.len1, lane);
        wave_copy_bytes(dst_seq + g.dst + g.len1, src_seq + g.src2, g.len2, lane);
        wave_copy_bytes(dst_qual + g.dst + g.len1, src_qual + g.src2, g.len2, lane);
    }
}

inline uint32_t self_wave_grid(uint64_t n) {  // one wave per item in workgroups of four, at most 2^16 workgroups (the kernels stride)
    const uint64_t g = (n + 3) / 4;
    return (uint32_t)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

hipError_t sr_self_launch_check(const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes, const hc_sr_pair* pairs, uint64_t n_pairs,
                                uint32_t min_overlap, uint32_t* status, SrSelfCheckCounters* counters, hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    if (((uintptr_t)seq | (uintptr_t)qual) & 15u) return hipErrorInvalidValue;
    // at most 2,048 workgroups, which stride: every workgroup ends in up to eight atomics on the same eight words
    const uint32_t grid = self_wave_grid(n_pairs) < 2048u ? self_wave_grid(n_pairs) : 2048u;
    hipLaunchKernelGGL(sr_self_check_kernel, dim3(grid), dim3(256), 0, s, seq, qual, n_bytes, pairs, n_pairs, min_overlap, status,
                       counters);
    return hipGetLastError();
}

hipError_t sr_self_launch_copy(const SrSelfSeg* segs, uint64_t n, const uint8_t* src_seq, const uint8_t* src_qual, uint8_t* dst_seq,
                               uint8_t* dst_qual, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sr_self_copy_kernel, dim3(self_wave_grid(n)), dim3(256), 0, s, segs, n, src_seq, src_qual, dst_seq, dst_qual);
    return hipGetLastError();
}

hipError_t sr_self_launch_scan(uint32_t n_cu, uint32_t lanes, const uint8_t* seq, const uint8_t* qual, const hc_sr_pair* pairs, const uint32_t* skip,
                               uint64_t n_pairs, const uint8_t* qmap, const double* lut, const double* inv_n, const SrSelfParams& prm, SrSelfScan* out,
                               hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    if (lanes == 0 || lanes > kSelfMaxChunk || (lanes & 63u)) return hipErrorInvalidValue;
    const bool lds_lut = (size_t)prm.lut_doubles * sizeof(double) <= kSelfLdsLutBytes;
    const size_t lds = (lds_lut ? (size_t)prm.lut_doubles * sizeof(double) : 0) + 2 * (size_t)kSelfCap * sizeof(uint16_t);
    const uint64_t most = (uint64_t)n_cu * (2048u / lanes);
    const uint32_t blocks = (uint32_t)(n_pairs < most ? n_pairs : most);
    if (lds_lut)
        hipLaunchKernelGGL(sr_self_scan_kernel<true>, dim3(blocks), dim3(lanes), lds, s, seq, qual, pairs, skip, n_pairs, qmap, lut, inv_n, prm, out);
    else
        hipLaunchKernelGGL(sr_self_scan_kernel<false>, dim3(blocks), dim3(lanes), lds, s, seq, qual, pairs, skip, n_pairs, qmap, lut, inv_n, prm, out);
    return hipGetLastError();
}

hipError_t sr_self_launch_merge(const uint8_t* seq, const uint8_t* qual, const hc_sr_pair* pairs, uint64_t n_pairs, const int32_t* mpos,
                                const uint64_t* off, uint64_t total, const double* terms, const uint8_t* table, uint8_t* out_seq, uint8_t* out_qual,
                                hipStream_t s) {
    if (total == 0 || n_pairs == 0) return hipSuccess;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sr_self_merge_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, seq, qual, pairs, n_pairs, mpos, off, total, terms, table, out_seq,
                       out_qual);
    return hipGetLastError();
}

}  // namespace hc
