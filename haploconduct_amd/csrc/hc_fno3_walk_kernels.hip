// hc_fno3_walk_kernels.hip — the device side of hc_fno3_from_originals (include/hcsr.h): the walk of SRBuilder::findNextOverlaps3 and
// nodeDictApproach (reference src/FindNextOverlaps3.cpp:20-134) over the kept dict.  One lane per item — a dict entry, a sorted place, a
// (pair, shared original) combination, a candidate pair — never a loop over an original's reads or a pair's originals, so that a hub
// original shared by 10^4 reads costs what its 5 * 10^7 combinations cost.  A lane finds its read, its run or its entry by bisection.
// Around them: two stable radix sorts, two ordered selections and two exclusive sums (hc_prims.hip).  The only atomics are a maximum and
// two counts, each once per block into a counter.
//
// f3w_keys1_kernel   entry e -> its read, the key original id << 32 | walk rank, the largest id.
// f3w_heads1_kernel  after the sort: sorted place p starts the run of an original.
// f3w_count_kernel   p -> the later places of its run: the combinations it owns.
// f3w_combos_kernel  after the sum: combination t -> its two places, the key rank of SR1 << b | rank of SR2, (d_l, d_r).
// f3w_heads2_kernel  after the stable sort: u starts the run of a pair (a candidate); u differs from its predecessor in the run.
// f3w_items_kernel   after the selection and the sum: candidate k -> the record fno3_deduce takes, and its row of the table.
// f3w_lines_kernel   after fno3_deduce: the candidates that wrote a line.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_device.h"
#include "hc_fno3_walk.h"

namespace hc {
namespace fno3w {
namespace {

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the largest j in [0, n) with a[j] <= x, for a[0] <= x < a[n] and ascending a
template <typename T>
__device__ inline uint64_t owner(const T* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void f3w_keys1_kernel(Dict D, Ranks K, Work W) {
    const uint64_t e = gid();
    __shared__ unsigned int top;
    if (threadIdx.x == 0) top = 0;
    __syncthreads();
    if (e < D.n_entries) {
        const uint64_t r = owner(D.off, D.n_reads, e);
        const uint32_t id = D.entries[e].id;
        W.key1_in[e] = (uint64_t)id << 32 | rank_of(K, r);
        W.val1_in[e] = (uint32_t)e;
        W.entry_read[e] = (uint32_t)r;
        atomicMax(&top, id);
    }
    __syncthreads();
    if (threadIdx.x == 0 && top) atomicMax(&W.counters[0], (unsigned long long)top);
}

__global__ __launch_bounds__(256) void f3w_heads1_kernel(Work W, uint64_t n_entries) {
    const uint64_t p = gid();
    if (p >= n_entries) return;
    W.head1[p] = p == 0 || (W.key1[p] >> 32) != (W.key1[p - 1] >> 32);
}

__global__ __launch_bounds__(256) void f3w_count_kernel(Work W, uint64_t n_entries) {
    const uint64_t p = gid();
    if (p > n_entries) return;
    uint64_t n = 0;
    if (p < n_entries) {
        const uint64_t n_orig = W.counters[1];  // (head1_pos[0] = 0 <= p)
        const uint64_t g = owner(W.head1_pos, n_orig, p);
        const uint64_t end = g + 1 < n_orig ? W.head1_pos[g + 1] : n_entries;
        n = end - 1 - p;
    }
    W.cnt[p] = n;
}

struct Places {
    uint64_t p, q;
};
// combination t: the entry at sorted place p with the (t - off[p])-th entry behind it in its run
__device__ inline Places places_of(const uint64_t* __restrict__ off, uint64_t n_entries, uint64_t t) {
    const uint64_t p = owner(off, n_entries, t);
    return Places{p, p + 1 + (t - off[p])};
}

__device__ inline bool paired_of(const ReadDesc* __restrict__ descs, uint32_t r) { return (descs[r].flags & kReadPaired) != 0; }

__global__ __launch_bounds__(256) void f3w_combos_kernel(Dict D, const ReadDesc* __restrict__ descs, Work W, uint64_t n_combos, int rank_bits) {
    const uint64_t t = gid();
    if (t >= n_combos) return;
    const Places c = places_of(W.cnt, D.n_entries, t);
    const uint32_t ea = W.val1[c.p], eb = W.val1[c.q];
    const uint64_t rank_a = (uint32_t)W.key1[c.p], rank_b = (uint32_t)W.key1[c.q];  // rank_a < rank_b: one run, sorted by rank
    W.key2_in[t] = rank_a << rank_bits | rank_b;
    W.val2_in[t] = (uint32_t)t;
    W.diff[t] = diff_of(D.entries[ea], D.entries[eb], paired_of(descs, W.entry_read[ea]) || paired_of(descs, W.entry_read[eb]));
}

__global__ __launch_bounds__(256) void f3w_heads2_kernel(Work W, uint64_t n_combos) {
    const uint64_t u = gid();
    if (u > n_combos) return;
    uint32_t differs = 0;
    if (u < n_combos) {
        const bool head = u == 0 || W.key2[u] != W.key2[u - 1];
        W.head2[u] = head;
        if (!head) {
            const Diff a = W.diff[W.val2[u]], b = W.diff[W.val2[u - 1]];
            differs = a.l != b.l || a.r != b.r;
        }
    }
    W.differs[u] = differs;
}

__global__ __launch_bounds__(256) void f3w_items_kernel(Dict D, const ReadDesc* __restrict__ descs, Work W, uint64_t n_combos, uint64_t n_cand,
                                                        FnoItem* __restrict__ items, hc_fno3_candidate* __restrict__ cands) {
    const uint64_t k = gid();
    __shared__ unsigned int ambiguous;
    if (threadIdx.x == 0) ambiguous = 0;
    __syncthreads();
    if (k < n_cand) {
        const uint64_t u = W.head2_pos[k], end = k + 1 < n_cand ? W.head2_pos[k + 1] : n_combos;
        const bool amb = W.differs[end] != W.differs[u];  // (exclusive sums; a head's own flag is 0)
        const Places c = places_of(W.cnt, D.n_entries, W.val2[u]);  // the first of the run: the smallest shared original
        const uint32_t ia = W.val1[c.p], ib = W.val1[c.q];
        const uint32_t ra = W.entry_read[ia], rb = W.entry_read[ib];
        const hc_sr_original ea = D.entries[ia], eb = D.entries[ib];
        const ReadDesc da = descs[ra], db = descs[rb];
        items[k] = item_of(ra, rb, ea, eb, da.len1, da.len2, (da.flags & kReadPaired) != 0, db.len1, db.len2, (db.flags & kReadPaired) != 0);
        cands[k] = hc_fno3_candidate{ra, rb, ea.id, amb ? HC_FNO3_CAND_AMBIGUOUS : 0u};
        if (amb) atomicAdd(&ambiguous, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && ambiguous) atomicAdd(&W.counters[3], (unsigned long long)ambiguous);
}

__global__ __launch_bounds__(256) void f3w_lines_kernel(const uint64_t* __restrict__ len, uint64_t n_cand, hc_fno3_candidate* __restrict__ cands) {
    const uint64_t k = gid();
    if (k < n_cand && len[k]) cands[k].flags |= HC_FNO3_CAND_LINE;
}

inline dim3 lanes(uint64_t n) { return dim3((uint32_t)((n + 255) / 256 ? (n + 255) / 256 : 1)); }  // (n < 2^32)

}  // namespace

hipError_t launch_keys1(Dict D, Ranks K, Work W, hipStream_t s) {
    hipLaunchKernelGGL(f3w_keys1_kernel, lanes(D.n_entries), dim3(256), 0, s, D, K, W);
    return hipGetLastError();
}
hipError_t launch_heads1(Work W, uint64_t n_entries, hipStream_t s) {
    hipLaunchKernelGGL(f3w_heads1_kernel, lanes(n_entries), dim3(256), 0, s, W, n_entries);
    return hipGetLastError();
}
hipError_t launch_count(Work W, uint64_t n_entries, hipStream_t s) {
    hipLaunchKernelGGL(f3w_count_kernel, lanes(n_entries + 1), dim3(256), 0, s, W, n_entries);
    return hipGetLastError();
}
hipError_t launch_combos(Dict D, const void* descs, Work W, uint64_t n_combos, int rank_bits, hipStream_t s) {
    hipLaunchKernelGGL(f3w_combos_kernel, lanes(n_combos), dim3(256), 0, s, D, (const ReadDesc*)descs, W, n_combos, rank_bits);
    return hipGetLastError();
}
hipError_t launch_heads2(Work W, uint64_t n_combos, hipStream_t s) {
    hipLaunchKernelGGL(f3w_heads2_kernel, lanes(n_combos + 1), dim3(256), 0, s, W, n_combos);
    return hipGetLastError();
}
hipError_t launch_items(Dict D, const void* descs, Work W, uint64_t n_combos, uint64_t n_cand, FnoItem* items, hc_fno3_candidate* cands, hipStream_t s) {
    hipLaunchKernelGGL(f3w_items_kernel, lanes(n_cand), dim3(256), 0, s, D, (const ReadDesc*)descs, W, n_combos, n_cand, items, cands);
    return hipGetLastError();
}
hipError_t launch_line_flags(const uint64_t* len, uint64_t n_cand, hc_fno3_candidate* cands, hipStream_t s) {
    hipLaunchKernelGGL(f3w_lines_kernel, lanes(n_cand), dim3(256), 0, s, len, n_cand, cands);
    return hipGetLastError();
}

}  // namespace fno3w
}  // namespace hc
