// hc_br_reduce_kernels.hip — the device part of hc_br_reduce (include/hcsr.h; hc_api_br.cpp drives it): the order-free half of the second
// half of BranchReduction::readBasedBranchReduction (reference src/BranchReduction.cpp:82-227, :1009-1272).
//
// br_red_triples_kernel  a lane per final_branch neighbour: Read::get_len() of its record's read1 and read2 and get_len(0), what the host's
//                        component walk asks getEdgeInfo for (:814-817, :909-912).  Bound: one record and four offsets per lane.
// br_red_rows_kernel     a lane per component edge: its row of the evidence tables by bisection over the (u, v) pairs, its list's length; an
//                        edge without a row marks its component (:1029-1031).  Bound: log2(rows) dependent loads.
// br_red_keys_kernel     a lane per evidence item: its component edge by bisection over the exclusive sum, the key component << id_bits | id,
//                        its own index as the value.  Bound: the bisection; the id itself is one coalesced load.
// (hc_prims)             one stable radix sort over id_bits + the component bits.
// br_red_unique_kernel   a lane per sorted item: equal to neither neighbour = in no other list of its component (a list does not repeat an
//                        id) -> 1 at the item's own index.  Bound: the scattered 8-byte store.
// (hc_prims)             one exclusive sum: items lie edge by edge, so an edge's count is a difference of two sums (no atomics).
// br_red_counts_kernel   a lane per component edge: that difference.
// br_red_decide_kernel   a lane per component: the general rule of :1243-1271 — an edge whose count is below min_evidence leaves, the component
//                        is kept if any edge stays.  Bound: a component's edges, read in order by one lane (components are small; a lane per
//                        edge would need atomics for `keep`).
// br_red_find_kernel     a wave per pair of edges_to_remove: lane 0 finds the first record u -> v of the target-ordered list by bisection,
//                        the wave walks adj_in[v] 64 entries at a time and takes the first u by ballot (OverlapGraph::removeEdge).  Bound:
//                        the in-list's length / 64 steps.  Not the lane / wave split of hc_trans_kernels.hip (a lane for a short list, the
//                        wave for a long one): every pair gets a wave, which idles 63 lanes during the bisection and on short in-lists;
//                        at 4·10^4 pairs that is 0.25 ms with the compaction (profiles/branch_reduce.md), so the split is not built.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_br.h"

namespace hc {
namespace br {
namespace {

constexpr uint32_t kBlock = 256;

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the largest j in [0, n) with a[j] <= x (a ascending, a[0] <= x)
__device__ inline uint64_t owner(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void br_red_triples_kernel(Graph g, Store st, Red R) {
    const uint64_t k = gid();
    if (k >= R.n_nb) return;
    const uint32_t rec = R.sl_rec[R.nb_sel[k]];
    int32_t len1 = 0, len2 = 0, olen = 0;
    if (rec < g.E) {
        const hc_edge_rec e = g.edges[rec];
        if (e.read1 < st.n_reads && e.read2 < st.n_reads) {
            len1 = (int32_t)(uint32_t)(st.off[st.first[e.read1 + 1]] - st.off[st.first[e.read1]]);
            len2 = (int32_t)(uint32_t)(st.off[st.first[e.read2 + 1]] - st.off[st.first[e.read2]]);
            olen = e.len0;
        } else {
            R.counters[kRedBadRead] = 1;
        }
    } else {
        R.counters[kRedBadRead] = 1;
    }
    R.tri[3 * k] = len1, R.tri[3 * k + 1] = len2, R.tri[3 * k + 2] = olen;
}

__global__ __launch_bounds__(256) void br_red_rows_kernel(Red R) {
    const uint64_t e = gid();
    if (e > R.n_ce) return;
    if (e == R.n_ce) {
        R.ce_len[e] = 0;
        return;
    }
    const uint32_t u = R.ce_u[e], v = R.ce_v[e];
    uint64_t lo = 0, hi = R.n_rows;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint32_t a = R.ev_edge[2 * mid], b = R.ev_edge[2 * mid + 1];
        if (a < u || (a == u && b < v)) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < R.n_rows && R.ev_edge[2 * lo] == u && R.ev_edge[2 * lo + 1] == v;
    R.ce_row[e] = found ? (uint32_t)lo : kNoRow;
    R.ce_len[e] = found ? R.ev_off[lo + 1] - R.ev_off[lo] : 0;
    if (!found) R.cm_no_row[R.ce_comp[e]] = 1;  // (every writer stores the same byte)
}

__global__ __launch_bounds__(256) void br_red_keys_kernel(Red R) {
    const uint64_t i = gid();
    if (i >= R.n_items) return;
    const uint64_t e = owner(R.ce_off, R.n_ce, i);  // (an empty list shares its offset with its successor: the largest j is the owner)
    const uint64_t id = R.ev_ids[R.ev_off[R.ce_row[e]] + (i - R.ce_off[e])];
    if (id >= R.id_limit) R.counters[kRedBadId] = 1;  // (the assert of :1068; the key's id field would not hold it)
    R.key_in[i] = (uint64_t)R.ce_comp[e] << R.id_bits | (id & ((1ull << R.id_bits) - 1));
    R.val_in[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void br_red_unique_kernel(Red R) {
    const uint64_t j = gid();
    if (j == R.n_items) R.uniq[j] = 0;
    if (j >= R.n_items) return;
    const uint64_t k = R.key[j];
    const bool alone = (j == 0 || R.key[j - 1] != k) && (j + 1 == R.n_items || R.key[j + 1] != k);
    R.uniq[R.val[j]] = alone ? 1 : 0;
}

__global__ __launch_bounds__(256) void br_red_counts_kernel(Red R) {
    const uint64_t e = gid();
    if (e >= R.n_ce) return;
    R.ce_count[e] = (uint32_t)(R.uniq[R.ce_off[e + 1]] - R.uniq[R.ce_off[e]]);
}

__global__ __launch_bounds__(256) void br_red_decide_kernel(Red R) {
    const uint64_t c = gid();
    if (c >= R.n_c) return;
    const int32_t min_evidence = R.cm_minev[c];
    bool keep = false;
    for (uint64_t e = R.cm_first[c]; e < R.cm_first[c + 1]; e++) {
        const bool below = (int32_t)R.ce_count[e] < min_evidence;  // :1251 (a count is below 2^31: items are)
        R.ce_remove[e] = below ? 1 : 0;
        keep |= !below;
    }
    R.cm_keep[c] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void br_red_find_kernel(Graph g, Red R) {
    const uint64_t p = gid() >> 6;  // (a block is four whole waves: all 64 lanes of a wave share p)
    const uint32_t lane = threadIdx.x & 63;
    if (p >= R.n_rm) return;
    const uint32_t u = R.rm_u[p], v = R.rm_v[p];
    if (u >= g.V || v >= g.V) {
        if (lane == 0) R.counters[kRedNotFound] = 1, R.rm_rec[p] = 0, R.rm_in[p] = 0;
        return;
    }
    if (lane == 0) {
        uint64_t lo = g.out_off[u], hi = g.out_off[u + 1];
        const uint64_t end = hi;
        while (lo < hi) {  // the first record whose target is not below v
            const uint64_t mid = lo + (hi - lo) / 2;
            if (g.edges[mid].v2 < v) lo = mid + 1;
            else hi = mid;
        }
        const bool found = lo < end && g.edges[lo].v2 == v;
        R.rm_rec[p] = found ? (uint32_t)lo : 0;
        if (!found) R.counters[kRedNotFound] = 1;
    }
    const uint64_t a = g.in_off[v], b = g.in_off[v + 1];
    bool done = false;
    for (uint64_t base = a; base < b && !done; base += 64) {  // (the trip count is wave-uniform: `done` comes from a ballot)
        const uint64_t q = base + lane;
        const unsigned long long hit = __ballot(q < b && g.in_nodes[q] == u);
        if (hit) {
            if (lane == 0) R.rm_in[p] = (uint32_t)(base + (uint64_t)__builtin_ctzll(hit));
            done = true;
        }
    }
    if (!done && lane == 0) R.rm_in[p] = 0, R.counters[kRedNotFound] = 1;
}

inline dim3 lanes(uint64_t n) {
    const uint64_t blocks = (n + kBlock - 1) / kBlock;
    return dim3((uint32_t)(blocks ? blocks : 1));
}

}  // namespace

#define HC_BR_LAUNCH(kernel, n, ...)                                           \
    do {                                                                       \
        hipLaunchKernelGGL(kernel, lanes(n), dim3(kBlock), 0, s, __VA_ARGS__); \
        return hipGetLastError();                                              \
    } while (0)

hipError_t launch_red_triples(const Graph& g, const Store& st, const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_triples_kernel, R.n_nb, g, st, R); }
hipError_t launch_red_rows(const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_rows_kernel, R.n_ce + 1, R); }
hipError_t launch_red_keys(const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_keys_kernel, R.n_items, R); }
hipError_t launch_red_unique(const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_unique_kernel, R.n_items + 1, R); }
hipError_t launch_red_counts(const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_counts_kernel, R.n_ce, R); }
hipError_t launch_red_decide(const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_decide_kernel, R.n_c, R); }
hipError_t launch_red_find(const Graph& g, const Red& R, hipStream_t s) { HC_BR_LAUNCH(br_red_find_kernel, R.n_rm * 64, g, R); }

}  // namespace br
}  // namespace hc
