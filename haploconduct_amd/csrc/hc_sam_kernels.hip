// hc_sam_kernels.hip — scripts/sam2overlaps.py's enumeration on the device.  The script keeps a list of active reads (:372-394, :528-554);
// here it is a closed form over the records in the script's order (per reference one stable sort by (position, kind, input order)):
//   * record i is processed iff pos_0 < len(ref) and i < min(n, 1 + #{k : pos_k < len(ref)})            (the loop tests the PREVIOUS position, :535)
//   * record i is evaluated against exactly the j < i with j == i - 1 or len_j - (pos_{i-1} - pos_j) >= min_overlap_len, in ascending j:
//     for a fixed j the range j < i <= e_j, where e_j comes from one bisection of the sorted positions.
// Layout over lanes: one wave per record i scans its window [lo_i, i) — lo_i the lowest j with e_j >= i, from a prefix maximum of e — 64
// records a step; a lane whose record is still active (e_j >= i) evaluates the pair (hc_sam_items.h: both CIGAR walks, the branch's second
// overlap), a ballot orders the lines of a step, the running count orders the steps: the lines of record i come out in ascending j with no
// atomics, and an exclusive sum over the records' counts places the records.  A window is mostly inactive records when one long read sits
// among short ones; the plan knows both sums (window: sum (i - lo_i), candidates: sum (e_j - j)) and refuses a lopsided input (hc_api_sam.cpp).
#include "hc_sam.h"
#include "hc_sam_items.h"

namespace hc {
namespace {
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;

__global__ __launch_bounds__(kBlock) void sam_keys_kernel(const hc_sam_aln* __restrict__ alns, const hc_sam_rec* __restrict__ recs, uint32_t n,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ iota) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const hc_sam_rec r = recs[k];
    const hc_sam_aln a = alns[r.first];
    const uint64_t biased = (uint64_t)(uint32_t)((int32_t)a.cpos + (int32_t)0x40000000);  // |cpos| < 2^30 (hc_set_sam_records)
    keys[k] = (uint64_t)a.ref << 32 | biased << 1 | (r.second != HC_SAM_NONE ? 1u : 0u);  // single first on a tie, :504
    iota[k] = k;
}

__global__ __launch_bounds__(kBlock) void sam_gather_kernel(const hc_sam_aln* __restrict__ alns, const hc_sam_rec* __restrict__ recs,
                                                            const uint32_t* __restrict__ perm, uint32_t n, int32_t* __restrict__ pos,
                                                            uint32_t* __restrict__ len, uint32_t* __restrict__ ref, hc_sam_rec* __restrict__ rec) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const hc_sam_rec r = recs[perm[i]];
    const hc_sam_aln a = alns[r.first];
    pos[i] = (int32_t)a.cpos;
    len[i] = a.len;
    ref[i] = a.ref;
    rec[i] = r;
}

// first index in [b, e) whose position is > v (upper bound) / >= v (lower bound)
__device__ __forceinline__ uint32_t upper_bound_pos(const int32_t* __restrict__ pos, uint32_t b, uint32_t e, int64_t v) {
    while (b < e) {
        const uint32_t m = b + (e - b) / 2;
        if ((int64_t)pos[m] <= v) b = m + 1;
        else e = m;
    }
    return b;
}

__global__ __launch_bounds__(kBlock) void sam_processed_kernel(const int32_t* __restrict__ pos, const uint32_t* __restrict__ seg_begin,
                                                               const uint64_t* __restrict__ ref_len, uint32_t n_refs, uint32_t* __restrict__ proc_end) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_refs) return;
    const uint32_t b = seg_begin[r], e = seg_begin[r + 1];
    uint32_t processed = 0;
    if (e > b) {
        const int64_t L = ref_len[r] > 0x7FFFFFFFull ? 0x7FFFFFFFll : (int64_t)ref_len[r];  // (positions are below 2^30)
        const uint32_t below = upper_bound_pos(pos, b, e, L - 1) - b;                       // #{k : pos_k < len(ref)}
        if (below > 0) processed = below + 1 < e - b ? below + 1 : e - b;
    }
    proc_end[r] = b + processed;
}

__global__ __launch_bounds__(kBlock) void sam_last_partner_kernel(SamSorted S, const uint32_t* __restrict__ seg_begin, const uint32_t* __restrict__ proc_end,
                                                                  int64_t mol, uint32_t* __restrict__ e_out, uint64_t* __restrict__ cand) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= S.n) return;
    const uint32_t r = S.ref[j];
    const uint32_t pe = proc_end[r];
    uint32_t e = j;
    if (j + 1 < pe) {  // record j + 1 is processed: j is its neighbour at least
        // i is evaluated against j iff pos_{i-1} <= pos_j + len_j - mol or i - 1 == j
        const int64_t bound = (int64_t)S.pos[j] + (int64_t)S.len[j] - mol;
        const uint32_t ub = upper_bound_pos(S.pos, j, seg_begin[r + 1], bound);  // i - 1 < ub
        e = ub > j + 1 ? ub : j + 1;
        if (e > pe - 1) e = pe - 1;
    }
    e_out[j] = e;
    cand[j] = e - j;
}

// ---- inclusive prefix maximum, three launches: a tile's maximum, the tiles' exclusive prefix (one block), the tile itself -------------
constexpr int kScanItems = 4;
constexpr uint32_t kScanTile = kBlock * kScanItems;

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
        v = v > o ? v : o;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void sam_tile_max_kernel(const uint32_t* __restrict__ e, uint32_t n, uint32_t* __restrict__ block_max) {
    __shared__ uint32_t part[kWavesPerBlock];
    const uint32_t base = blockIdx.x * kScanTile;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        const uint32_t i = base + k * kBlock + threadIdx.x;
        if (i < n) v = v > e[i] ? v : e[i];
    }
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = part[0];
        for (int w = 1; w < kWavesPerBlock; w++) m = m > part[w] ? m : part[w];
        block_max[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(kBlock) void sam_tiles_prefix_kernel(uint32_t* __restrict__ block_max, uint32_t n_tiles) {  // one block
    __shared__ uint32_t tot[kBlock];
    const uint32_t per = (n_tiles + kBlock - 1) / kBlock;
    const uint32_t b = threadIdx.x * per, e = b + per < n_tiles ? b + per : n_tiles;
    uint32_t m = 0;
    for (uint32_t t = b; t < e; t++) m = m > block_max[t] ? m : block_max[t];
    tot[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {  // exclusive prefix of the threads' maxima
        uint32_t run = 0;
        for (int t = 0; t < kBlock; t++) {
            const uint32_t v = tot[t];
            tot[t] = run;
            run = run > v ? run : v;
        }
    }
    __syncthreads();
    uint32_t run = tot[threadIdx.x];
    for (uint32_t t = b; t < e; t++) {
        const uint32_t v = block_max[t];
        block_max[t] = run;  // the maximum of every tile in front of t
        run = run > v ? run : v;
    }
}

__global__ __launch_bounds__(kBlock) void sam_tile_scan_kernel(const uint32_t* __restrict__ e, uint32_t n, const uint32_t* __restrict__ block_prefix,
                                                               uint32_t* __restrict__ m_out) {
    __shared__ uint32_t tot[kBlock];
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;  // a thread's items are neighbours
    uint32_t v[kScanItems];
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        const uint32_t x = base + k < n ? e[base + k] : 0u;
        run = run > x ? run : x;
        v[k] = run;
    }
    tot[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t r = block_prefix[blockIdx.x];
        for (int t = 0; t < kBlock; t++) {
            const uint32_t x = tot[t];
            tot[t] = r;
            r = r > x ? r : x;
        }
    }
    __syncthreads();
    const uint32_t carry = tot[threadIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; k++)
        if (base + k < n) m_out[base + k] = v[k] > carry ? v[k] : carry;
}

__global__ __launch_bounds__(kBlock) void sam_window_kernel(SamSorted S, const uint32_t* __restrict__ seg_begin, const uint32_t* __restrict__ proc_end,
                                                            const uint32_t* __restrict__ m, uint32_t* __restrict__ lo, uint64_t* __restrict__ win) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= S.n) return;
    const uint32_t r = S.ref[i];
    uint32_t b = seg_begin[r], e = i;
    if (i >= proc_end[r]) b = i;  // not processed: nothing to scan
    while (b < e) {               // the first j with max(e_0 .. e_j) >= i: the first j with e_j >= i
        const uint32_t mid = b + (e - b) / 2;
        if (m[mid] >= i) e = mid;
        else b = mid + 1;
    }
    lo[i] = b;
    win[i] = i - b;
}

// One wave per record i.  WRITE = false: cnt[i] = its lines.  WRITE = true: its lines with file index in [first_line, first_line + n_lines)
// go to out[index - first_line]; the record's first line has index off[i].
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void sam_pairs_kernel(SamSorted S, const hc_sam_aln* __restrict__ alns, const hc_sam_op* __restrict__ ops,
                                                           const uint32_t* __restrict__ lo, const uint32_t* __restrict__ e, int64_t mol, uint32_t i0,
                                                           uint32_t i1, uint64_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint64_t first_line,
                                                           uint64_t n_lines, hc_line_rec* __restrict__ out, unsigned long long* __restrict__ status) {
    const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (wave >= i1 - i0) return;  // (uniform over the wave)
    const uint32_t i = i0 + wave;
    const hc_sam_rec ri = S.rec[i];
    const SamPair record{ri.first, ri.second, ri.reverse};
    uint64_t at = WRITE ? off[i] : 0;  // file index of the next line of this record
    const uint64_t end_line = first_line + n_lines;
    if (WRITE && (off[i + 1] <= first_line || at >= end_line)) return;
    uint32_t bad = 0;
    for (uint32_t j0 = lo[i]; j0 < i; j0 += 64) {
        const uint32_t j = j0 + lane;
        bool emitted = false;
        hc_line_rec line;
        if (j < i && e[j] >= i) {  // still in the script's list of active reads
            const hc_sam_rec rj = S.rec[j];
            const SamPair read{rj.first, rj.second, rj.reverse};
            const bool same_id = ri.second != HC_SAM_NONE && rj.second != HC_SAM_NONE && alns[rj.first].id == alns[ri.second].id;
            uint32_t src[2], err = 0;
            emitted = sam_pair_line(alns, ops, record, read, mol, same_id, line, src, err);
            if (err) bad |= err == kSamRange ? (uint32_t)kSamStatusRange : (uint32_t)kSamStatusScript;
        }
        const unsigned long long mask = __ballot(emitted);
        if (WRITE && emitted) {
            const uint64_t idx = at + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (idx >= first_line && idx < end_line) out[idx - first_line] = line;
        }
        at += (uint64_t)__popcll(mask);
        if (WRITE && at >= end_line) break;  // (uniform)
    }
    if (!WRITE) {
        if (lane == 0) cnt[i] = at;
        if (bad) atomicOr(status, (unsigned long long)bad);
    }
}

__global__ void sam_owner_range_kernel(const uint64_t* __restrict__ off, uint32_t n, uint64_t first_line, uint64_t n_lines, uint32_t* __restrict__ range) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // owner of line x: the last i with off[i] <= x (records without lines share an offset with their successor and own nothing)
    auto owner = [&](uint64_t x) {
        uint32_t b = 0, e = n;  // first i in [0, n] with off[i] > x, minus one
        while (b < e) {
            const uint32_t m = b + (e - b) / 2;
            if (off[m] <= x) b = m + 1;
            else e = m;
        }
        return b - 1;
    };
    if (n_lines == 0 || first_line >= off[n]) {
        range[0] = range[1] = 0;
        return;
    }
    const uint64_t last = first_line + n_lines - 1 < off[n] - 1 ? first_line + n_lines - 1 : off[n] - 1;
    range[0] = owner(first_line);
    range[1] = owner(last) + 1;
}

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
}  // namespace

hipError_t sam_keys(const hc_sam_aln* alns, const hc_sam_rec* recs, uint32_t n, uint64_t* keys, uint32_t* iota, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(sam_keys_kernel, grid_for(n), dim3(kBlock), 0, s, alns, recs, n, keys, iota);
    return hipGetLastError();
}
hipError_t sam_gather(const hc_sam_aln* alns, const hc_sam_rec* recs, const uint32_t* perm, uint32_t n, int32_t* pos, uint32_t* len, uint32_t* ref,
                      hc_sam_rec* rec, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(sam_gather_kernel, grid_for(n), dim3(kBlock), 0, s, alns, recs, perm, n, pos, len, ref, rec);
    return hipGetLastError();
}
hipError_t sam_processed(const int32_t* pos, const uint32_t* seg_begin, const uint64_t* ref_len, uint32_t n_refs, uint32_t* proc_end, hipStream_t s) {
    if (!n_refs) return hipSuccess;
    hipLaunchKernelGGL(sam_processed_kernel, grid_for(n_refs), dim3(kBlock), 0, s, pos, seg_begin, ref_len, n_refs, proc_end);
    return hipGetLastError();
}
hipError_t sam_last_partner(const SamSorted& S, const uint32_t* seg_begin, const uint32_t* proc_end, int64_t mol, uint32_t* e, uint64_t* cand, hipStream_t s) {
    if (!S.n) return hipSuccess;
    hipLaunchKernelGGL(sam_last_partner_kernel, grid_for(S.n), dim3(kBlock), 0, s, S, seg_begin, proc_end, mol, e, cand);
    return hipGetLastError();
}
hipError_t sam_prefix_max(const uint32_t* e, uint32_t n, uint32_t* m, uint32_t* block_max, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint32_t tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(sam_tile_max_kernel, dim3(tiles), dim3(kBlock), 0, s, e, n, block_max);
    hipLaunchKernelGGL(sam_tiles_prefix_kernel, dim3(1), dim3(kBlock), 0, s, block_max, tiles);
    hipLaunchKernelGGL(sam_tile_scan_kernel, dim3(tiles), dim3(kBlock), 0, s, e, n, block_max, m);
    return hipGetLastError();
}
hipError_t sam_window(const SamSorted& S, const uint32_t* seg_begin, const uint32_t* proc_end, const uint32_t* m, uint32_t* lo, uint64_t* win, hipStream_t s) {
    if (!S.n) return hipSuccess;
    hipLaunchKernelGGL(sam_window_kernel, grid_for(S.n), dim3(kBlock), 0, s, S, seg_begin, proc_end, m, lo, win);
    return hipGetLastError();
}
hipError_t sam_count(const SamSorted& S, const hc_sam_aln* alns, const hc_sam_op* ops, const uint32_t* lo, const uint32_t* e, int64_t mol, uint64_t* cnt,
                     unsigned long long* status, hipStream_t s) {
    if (!S.n) return hipSuccess;
    hipLaunchKernelGGL((sam_pairs_kernel<false>), dim3((S.n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, s, S, alns, ops, lo, e, mol, 0u, S.n, cnt,
                       (const uint64_t*)nullptr, (uint64_t)0, (uint64_t)0, (hc_line_rec*)nullptr, status);
    return hipGetLastError();
}
hipError_t sam_owner_range(const uint64_t* off, uint32_t n, uint64_t first_line, uint64_t n_lines, uint32_t* range, hipStream_t s) {
    hipLaunchKernelGGL(sam_owner_range_kernel, dim3(1), dim3(64), 0, s, off, n, first_line, n_lines, range);
    return hipGetLastError();
}
hipError_t sam_write(const SamSorted& S, const hc_sam_aln* alns, const hc_sam_op* ops, const uint32_t* lo, const uint32_t* e, const uint64_t* off, int64_t mol,
                     uint32_t i0, uint32_t i1, uint64_t first_line, uint64_t n_lines, hc_line_rec* out, hipStream_t s) {
    if (i1 <= i0 || !n_lines) return hipSuccess;
    hipLaunchKernelGGL((sam_pairs_kernel<true>), dim3((i1 - i0 + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, s, S, alns, ops, lo, e, mol, i0, i1,
                       (uint64_t*)nullptr, off, first_line, n_lines, out, (unsigned long long*)nullptr);
    return hipGetLastError();
}

}  // namespace hc
