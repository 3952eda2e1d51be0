// hc_trans_kernels.hip — OverlapGraph::removeInclusions and removeTransitiveEdges (src/GraphAlgos.cpp:20-48, 746-833,
// 938-1077), removeTips (:543-637) and removeBranches (:835-936; described where their kernels start) on the device graph,
// for gfx950.
//
// removeTransitiveEdges:
//   target order        every out-list stably sorted by target (radix sort of (source, target), positions as values);
//                       lists of more than 16 entries with a repeated target are listed and the host puts std::sort's
//                       order there (target_sort_perm, hc_trans.h) — a stable sort is std::sort's order everywhere else
//   sorted in-lists     the in-entries sorted by (target, source) (sortAdjLists(adj_in)), positions as values
//   intersection        edge (u, w) is transitive iff out(u) and in(w) share an element: one wave per 64 consecutive
//                       edges, for each edge the lanes take 64 entries of the shorter list at a time and binary-search
//                       the longer one; a ballot ends the search at the first hit.  No lane walks a list on its own,
//                       so a hub costs its length / 64 wave steps per edge, whatever its degree.
//   passes 2..k         the same test on the compacted transitive edges (a subset of sorted lists stays sorted)
//   branch reduction    per-vertex atomicMax of ovlen on the out side and the in side, then one flagging pass
//   removal             the rebuild branch (new lists without T_k and without every edge of a pair in D, adj_in in
//                       vertex order) or the removeEdge branch (T_k, then the first remaining edge of every D pair,
//                       adj_in keeping its order), as the reference chooses
// removeInclusions: group sizes, a scan, the group writes, then the first edge of every pair touching an inclusion
// vertex leaves adj_out and its first entry leaves adj_in.
// All of it is bandwidth-bound integer work; sorts, scans and selections are hc_prims.hip's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/hcedge.h"
#include "hc_prims.h"
#include "hc_trans.h"
#include "host/ExtLen.h"

namespace hc {
namespace trans {

namespace {

constexpr int kBlock = 256;

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, 1u << 16))); }

#define TRY(x)                                 \
    do {                                       \
        const hipError_t e_ = (x);             \
        if (e_ != hipSuccess) return e_;       \
    } while (0)

// Scratch carving: the same sequence of take() calls sizes the scratch (base == nullptr) and carves it.
struct Carve {
    char* base;
    size_t used = 0;
    template <typename T>
    T* take(uint64_t n) {
        const size_t at = (used + 255) & ~(size_t)255;
        used = at + (size_t)(n ? n : 1) * sizeof(T);
        return base ? (T*)(base + at) : nullptr;
    }
};

struct Work {
    uint32_t *src, *tgt_orig, *iota, *perm, *tgt, *in_owner, *in_pos, *first, *idx;
    uint64_t *key_a, *key_b, *key_c;
    uint32_t *lsrc[2], *ltgt[2], *lpos[2], *lin_src;
    unsigned long long *lout_off, *lin_off, *hist, *counters;
    uint8_t *flags, *in_t, *in_d, *pair_d, *keep, *in_keep, *tied;
    int *max_out, *max_in;
    uint32_t* tied_list;
    void* prims;
    size_t prims_bytes;
};

size_t prims_bytes_for(uint64_t E, uint64_t V) {
    size_t b = prims::sort_temp_bytes(E ? E : 1, sizeof(uint64_t), sizeof(uint32_t));
    b = std::max(b, prims::scan_temp_bytes(V + 2, sizeof(uint64_t)));
    b = std::max(b, prims::select_temp_bytes(std::max<uint64_t>(E, V) + 1));
    return b;
}

Work layout(Carve& c, uint64_t E, uint64_t V) {
    Work w;
    w.src = c.take<uint32_t>(E);
    w.tgt_orig = c.take<uint32_t>(E);
    w.iota = c.take<uint32_t>(E);
    w.perm = c.take<uint32_t>(E);
    w.tgt = c.take<uint32_t>(E);
    w.in_owner = c.take<uint32_t>(E);
    w.in_pos = c.take<uint32_t>(E);
    w.first = c.take<uint32_t>(E);
    w.idx = c.take<uint32_t>(E);
    w.key_a = c.take<uint64_t>(E);
    w.key_b = c.take<uint64_t>(E);
    w.key_c = c.take<uint64_t>(E);
    for (int k = 0; k < 2; k++) {
        w.lsrc[k] = c.take<uint32_t>(E);
        w.ltgt[k] = c.take<uint32_t>(E);
        w.lpos[k] = c.take<uint32_t>(E);
    }
    w.lin_src = c.take<uint32_t>(E);
    w.lout_off = c.take<unsigned long long>(V + 2);
    w.lin_off = c.take<unsigned long long>(V + 2);
    w.hist = c.take<unsigned long long>(V + 2);
    w.counters = c.take<unsigned long long>(8);
    w.flags = c.take<uint8_t>(E);
    w.in_t = c.take<uint8_t>(E);
    w.in_d = c.take<uint8_t>(E);
    w.pair_d = c.take<uint8_t>(E);
    w.keep = c.take<uint8_t>(E);
    w.in_keep = c.take<uint8_t>(E);
    w.tied = c.take<uint8_t>(V + 1);
    w.max_out = c.take<int>(V + 1);
    w.max_in = c.take<int>(V + 1);
    w.tied_list = c.take<uint32_t>(V + 1);
    w.prims_bytes = prims_bytes_for(E, V);
    w.prims = c.take<char>(w.prims_bytes);
    return w;
}

// ---- kernels -------------------------------------------------------------------------------------------------------

// owner[i] = the list that holds entry i (binary search of the offsets), vals[i] = i
__global__ void k_owner(const unsigned long long* __restrict__ off, uint32_t V, uint32_t n, uint32_t* __restrict__ owner,
                        uint32_t* __restrict__ iota) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = V;  // the last v with off[v] <= i
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid;
            else hi = mid;
        }
        owner[i] = lo;
        if (iota) iota[i] = i;
    }
}

__global__ void k_out_keys(const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ src, uint32_t n, uint32_t* __restrict__ tgt_orig,
                           uint64_t* __restrict__ key) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)E[i].v2;
        tgt_orig[i] = t;
        key[i] = ((uint64_t)src[i] << 32) | t;
    }
}

__global__ void k_pair_keys(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo, uint32_t n, uint64_t* __restrict__ key) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) key[i] = ((uint64_t)hi[i] << 32) | lo[i];
}

__global__ void k_low32(const uint64_t* __restrict__ key, uint32_t n, uint32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = (uint32_t)key[i];
}

// tied[u] = 1 for a list of more than 16 entries whose target-sorted form repeats a target (std::sort's insertion
// sort leaves shorter lists stable)
__global__ void k_tied(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const unsigned long long* __restrict__ off, uint32_t n,
                       uint8_t* __restrict__ tied) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t u = src[i];
        if (i > off[u] && tgt[i] == tgt[i - 1] && off[u + 1] - off[u] > 16) tied[u] = 1;
    }
}

// one block per listed list: its targets in list order -> pack[pack_off[t] ..)
__global__ void k_pack_lists(const uint32_t* __restrict__ list, uint32_t n_lists, const unsigned long long* __restrict__ off,
                             const uint32_t* __restrict__ pack_off, const uint32_t* __restrict__ tgt_orig, uint32_t* __restrict__ pack) {
    for (uint32_t t = blockIdx.x; t < n_lists; t += gridDim.x) {
        const uint64_t o = off[list[t]];
        const uint32_t n = pack_off[t + 1] - pack_off[t];
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) pack[pack_off[t] + k] = tgt_orig[o + k];
    }
}

// ... and the host's permutations (positions within the list) back into perm
__global__ void k_unpack_perm(const uint32_t* __restrict__ list, uint32_t n_lists, const unsigned long long* __restrict__ off,
                              const uint32_t* __restrict__ pack_off, const uint32_t* __restrict__ pack, uint32_t* __restrict__ perm) {
    for (uint32_t t = blockIdx.x; t < n_lists; t += gridDim.x) {
        const uint64_t o = off[list[t]];
        const uint32_t n = pack_off[t + 1] - pack_off[t];
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
            const uint32_t p = pack[pack_off[t] + k];
            if (p < n) perm[o + k] = (uint32_t)o + p;
        }
    }
}

__global__ void k_histogram(const uint32_t* __restrict__ key, uint32_t n, unsigned long long* __restrict__ hist) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) atomicAdd(&hist[key[i]], 1ull);
}

__device__ __forceinline__ uint32_t lower_bound_u64(const uint64_t* a, uint32_t n, uint64_t x) {
    uint32_t lo = 0;
    while (n > 0) {
        const uint32_t h = n >> 1;
        if (a[lo + h] < x) {
            lo += h + 1;
            n -= h + 1;
        } else {
            n = h;
        }
    }
    return lo;
}

__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t x) {
    uint32_t lo = 0;
    while (n > 0) {
        const uint32_t h = n >> 1;
        if (a[lo + h] < x) {
            lo += h + 1;
            n -= h + 1;
        } else {
            n = h;
        }
    }
    return lo;
}

// findTransEdges (:746-777) with removeTrans = false.  One wave per 64 consecutive edges; per edge the wave intersects
// out(u) (out_val[out_off[u] ..)) with in(w) (in_val[in_off[w] ..)): 64 entries of the shorter list at a time, each lane
// binary-searching the longer one, the first ballot with a hit ends it.
__global__ void __launch_bounds__(kBlock) k_intersect(const uint32_t* __restrict__ esrc, const uint32_t* __restrict__ etgt, uint32_t m,
                                                      const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ out_val,
                                                      const unsigned long long* __restrict__ in_off, const uint32_t* __restrict__ in_val,
                                                      uint8_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); (uint64_t)chunk * 64 < m; chunk += n_waves) {
        const uint32_t base = chunk * 64;
        const uint32_t cnt = min(64u, m - base);
        // lane j holds edge base + j's endpoints; the wave walks the edges one by one with them broadcast
        const uint32_t my_u = lane < cnt ? esrc[base + lane] : 0, my_w = lane < cnt ? etgt[base + lane] : 0;
        uint8_t my_flag = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t u = __shfl(my_u, j), w = __shfl(my_w, j);
            const uint64_t a0 = out_off[u], a1 = out_off[u + 1], b0 = in_off[w], b1 = in_off[w + 1];
            const uint32_t na = (uint32_t)(a1 - a0), nb = (uint32_t)(b1 - b0);
            const bool a_short = na <= nb;
            const uint32_t* S = a_short ? out_val + a0 : in_val + b0;
            const uint32_t* L = a_short ? in_val + b0 : out_val + a0;
            const uint32_t ns = a_short ? na : nb, nl = a_short ? nb : na;
            bool hit = false;
            if (ns && nl && S[0] <= L[nl - 1] && L[0] <= S[ns - 1]) {
                for (uint32_t k = 0; k < ns && !hit; k += 64) {
                    bool mine = false;
                    if (k + lane < ns) {
                        const uint32_t x = S[k + lane];
                        const uint32_t at = lower_bound_u32(L, nl, x);
                        mine = at < nl && L[at] == x;
                    }
                    hit = __ballot(mine) != 0;
                }
            }
            if (lane == j) my_flag = hit ? 1 : 0;
        }
        if (lane < cnt) flag[base + lane] = my_flag;
    }
}

__global__ void k_gather_level(const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ count, const uint32_t* __restrict__ s0,
                               const uint32_t* __restrict__ t0, const uint32_t* __restrict__ p0, uint32_t* __restrict__ s1, uint32_t* __restrict__ t1,
                               uint32_t* __restrict__ p1) {
    const uint32_t n = (uint32_t)*count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t k = idx[i];
        s1[i] = s0[k];
        t1[i] = t0[k];
        p1[i] = p0 ? p0[k] : k;
    }
}

__global__ void k_mark(const uint32_t* __restrict__ pos, uint32_t n, uint8_t* __restrict__ mark) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) mark[pos[i]] = 1;
}

// first[i]: the position of the first entry of i's (source, target) run in the target-sorted list — getEdgeInfo's edge
// (a binary search of the list: a pair repeated r times costs log r, not r, however many copies a caller's graph holds)
__global__ void k_first(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const unsigned long long* __restrict__ off, uint32_t n,
                        uint32_t* __restrict__ first) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t lo = off[src[i]];
        first[i] = (uint32_t)lo + lower_bound_u32(tgt + lo, (uint32_t)(i - lo), tgt[i]);
    }
}

__global__ void k_fill_int(int* __restrict__ a, uint32_t n, int v) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) a[i] = v;
}

// branch reduction (:968-993): every transitive (u, w) raises max_out[u] and max_in[w] to ovlen = len0 of its first edge
__global__ void k_branch_max(const uint32_t* __restrict__ tpos, uint32_t nt, const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt,
                             const uint32_t* __restrict__ first, const uint32_t* __restrict__ perm, const hc_edge_rec* __restrict__ E,
                             int* __restrict__ max_out, int* __restrict__ max_in) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += gridDim.x * blockDim.x) {
        const uint32_t p = tpos[i];
        const int ov = E[perm[first[p]]].len0;
        atomicMax(&max_out[src[p]], ov);
        atomicMax(&max_in[tgt[p]], ov);
    }
}

// the pairs of D: (u, v) when some u -> v edge has len0 <= max_out[u]; (x, w) when the first x -> w edge has len0 <= max_in[w]
__global__ void k_branch_pairs(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ first,
                               const uint32_t* __restrict__ perm, const hc_edge_rec* __restrict__ E, uint32_t n, const int* __restrict__ max_out,
                               const int* __restrict__ max_in, uint8_t* __restrict__ pair_d) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t f = first[i];
        if (E[perm[i]].len0 <= max_out[src[i]] || E[perm[f]].len0 <= max_in[tgt[i]]) pair_d[f] = 1;
    }
}

__global__ void k_spread_pairs(const uint32_t* __restrict__ first, const uint8_t* __restrict__ pair_d, uint32_t n, uint8_t* __restrict__ in_d) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) in_d[i] = pair_d[first[i]];
}

__device__ __forceinline__ void wave_count(bool pred, unsigned long long* counter) {
    const unsigned long long b = __ballot(pred);  // every lane of the wave is here: the loops that call this run in step
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (unsigned long long)__popcll(b));
}

// which target-sorted out entries survive; counts[0] += deletions (branch edges for the rebuild branch, D pairs
// removed for the removeEdge branch)
__global__ void k_keep_out(const uint8_t* __restrict__ in_t, const uint8_t* __restrict__ in_d, const uint32_t* __restrict__ first, uint32_t n,
                           uint32_t rebuild, uint8_t* __restrict__ keep, unsigned long long* __restrict__ deleted) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (n + stride - 1) / stride * stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        bool del = false;
        if (i < n) {
            const bool t = in_t[i] != 0, d = in_d[i] != 0;
            // removeEdge branch: T_k goes entirely (every copy of a pair is in T_k or none is); a D pair loses its first edge
            del = !t && d && (rebuild || first[i] == i);
            keep[i] = !t && !del;
        }
        wave_count(del, deleted);
    }
}

// removeEdge branch, adj_in: the in-entry at sorted place j (key (target, source), value = its place in adj_in) goes when
// its rank among the equal entries of its list is below the number of edges its pair lost
__global__ void k_keep_in_removed(const uint64_t* __restrict__ key, const uint32_t* __restrict__ in_pos, uint32_t n,
                                  const unsigned long long* __restrict__ in_off, const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ in_t,
                                  const uint8_t* __restrict__ in_d, uint8_t* __restrict__ in_keep) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint64_t k = key[j];
        const uint32_t x = (uint32_t)k, y = (uint32_t)(k >> 32);
        // the sorted entries of in(y) occupy [in_off[y], in_off[y + 1]); the rank is j's distance from the first equal one
        const uint64_t i0 = in_off[y];
        const uint32_t rank = (uint32_t)(j - i0) - lower_bound_u64(key + i0, (uint32_t)(j - i0), k);
        const uint64_t o0 = out_off[x];
        const uint32_t f = (uint32_t)o0 + lower_bound_u32(tgt + o0, (uint32_t)(out_off[x + 1] - o0), y);
        const bool found = f < out_off[x + 1] && tgt[f] == y;
        const uint32_t removed = !found ? 0u : in_t[f] ? 0xffffffffu : (in_d[f] ? 1u : 0u);
        in_keep[in_pos[j]] = rank >= removed;
    }
}

__global__ void k_gather_out(const uint32_t* __restrict__ kidx, const unsigned long long* __restrict__ count, const uint32_t* __restrict__ perm,
                             const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ seq, hc_edge_rec* __restrict__ E_out,
                             uint32_t* __restrict__ seq_out, uint32_t* __restrict__ src_out, const uint32_t* __restrict__ src) {
    const uint32_t n = (uint32_t)*count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t p = kidx[i];
        const uint32_t e = perm ? perm[p] : p;
        E_out[i] = E[e];
        seq_out[i] = seq[e];
        src_out[i] = src[p];
    }
}

__global__ void k_gather_u32(const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ count, const uint32_t* __restrict__ in,
                             uint32_t* __restrict__ out) {
    const uint32_t n = (uint32_t)*count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = in[idx[i]];
}

__global__ void k_count_to_u32(const unsigned long long* __restrict__ count, uint32_t* __restrict__ out) { *out = (uint32_t)*count; }

// removeInclusions: group sizes (out-degree + in-degree of a marked vertex)
__global__ void k_group_sizes(const uint8_t* __restrict__ incl, const unsigned long long* __restrict__ out_off,
                              const unsigned long long* __restrict__ in_off, uint32_t V, unsigned long long* __restrict__ sizes) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v <= V; v += gridDim.x * blockDim.x)
        sizes[v] = (v < V && incl[v]) ? (out_off[v + 1] - out_off[v]) + (in_off[v + 1] - in_off[v]) : 0;
}

__global__ void k_group_off(const uint32_t* __restrict__ gv, const unsigned long long* __restrict__ count, const unsigned long long* __restrict__ start,
                            uint32_t V, unsigned long long* __restrict__ group_off) {
    const uint32_t n = (uint32_t)*count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) group_off[i] = i < n ? start[gv[i]] : start[V];
}

// the out part of every group (records in list order), and which out entries leave: the first edge of every pair that
// touches a marked vertex (stable target order: the run's first entry is the first in list order)
__global__ void k_incl_out(const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt_orig, uint32_t n,
                           const uint8_t* __restrict__ incl, const unsigned long long* __restrict__ out_off, const unsigned long long* __restrict__ start,
                           hc_edge_rec* __restrict__ group_edges) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t u = src[i];
        if (incl[u]) group_edges[start[u] + (i - out_off[u])] = E[i];
    }
}

__global__ void k_incl_keep_out(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ perm,
                                const unsigned long long* __restrict__ out_off, uint32_t n, const uint8_t* __restrict__ incl,
                                uint8_t* __restrict__ keep, unsigned long long* __restrict__ removed) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (n + stride - 1) / stride * stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        bool del = false;
        if (i < n) {
            const uint32_t u = src[i], w = tgt[i];
            del = (incl[u] || incl[w]) && !(i > out_off[u] && tgt[i - 1] == w);
            keep[perm[i]] = !del;
        }
        wave_count(del, removed);
    }
}

// the in part of every group: for in-entry q of a marked v (x = in_nodes[q]), the first x -> v edge in x's list order;
// and which in-entries leave: the first occurrence of x in in(v) when x or v is marked
__global__ void k_incl_in(const uint64_t* __restrict__ key, const uint32_t* __restrict__ in_pos, uint32_t n, const unsigned long long* __restrict__ in_off,
                          const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ perm,
                          const hc_edge_rec* __restrict__ E, const uint8_t* __restrict__ incl, const unsigned long long* __restrict__ start,
                          hc_edge_rec* __restrict__ group_edges, uint8_t* __restrict__ in_keep) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint64_t k = key[j];
        const uint32_t x = (uint32_t)k, v = (uint32_t)(k >> 32);
        const uint32_t q = in_pos[j];
        const bool first_of_pair = j == 0 || key[j - 1] != k;
        in_keep[q] = !((incl[x] || incl[v]) && first_of_pair);
        if (incl[v]) {
            const uint64_t o0 = out_off[x];
            const uint32_t f = (uint32_t)o0 + lower_bound_u32(tgt + o0, (uint32_t)(out_off[x + 1] - o0), v);
            if (f < out_off[x + 1] && tgt[f] == v)  // hc_graph_load checks that adj_in and adj_out hold the same pairs
                group_edges[start[v] + (out_off[v + 1] - out_off[v]) + (q - in_off[v])] = E[perm[f]];
        }
    }
}

// hc_graph_load's checks: every record in the list of its vertex1, every id < V; counter += offenders
__global__ void k_check_ids(const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ in_nodes, uint32_t n,
                            uint32_t V, unsigned long long* __restrict__ bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (E[i].v1 != src[i] || E[i].v2 >= V || in_nodes[i] >= V) atomicAdd(bad, 1ull);
}

// ... and adj_in holding the same (source, target) pairs as adj_out: the two sorted key arrays are equal
__global__ void k_compare_keys(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint32_t n, unsigned long long* __restrict__ bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (a[i] != b[i]) atomicAdd(bad, 1ull);
}

// ---- host-side steps ---------------------------------------------------------------------------------------------------

// off[0..V] from a histogram of the keys (every key < V)
hipError_t offsets_of(const uint32_t* keys, uint32_t n, uint32_t V, unsigned long long* off, const Work& w, hipStream_t s) {
    TRY(hipMemsetAsync(w.hist, 0, ((size_t)V + 1) * sizeof(unsigned long long), s));
    if (n) {
        hipLaunchKernelGGL(k_histogram, grid_for(n), dim3(kBlock), 0, s, keys, n, w.hist);
        TRY(hipGetLastError());
    }
    return prims::exclusive_sum(w.prims, w.prims_bytes, (const uint64_t*)w.hist, (uint64_t*)off, (uint64_t)V + 1, s);
}

int key_bits(uint32_t V) {
    int b = 1;
    while (b < 32 && (1ull << b) < V) b++;
    return b;
}

// sorted in-lists of the edges (esrc[i], etgt[i]): lin_src (sources ascending within a list) and lin_off
hipError_t sorted_in_lists(const uint32_t* esrc, const uint32_t* etgt, uint32_t m, uint32_t V, const Work& w, hipStream_t s) {
    TRY(offsets_of(etgt, m, V, w.lin_off, w, s));
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_pair_keys, grid_for(m), dim3(kBlock), 0, s, etgt, esrc, m, w.key_a);
    TRY(hipGetLastError());
    TRY(prims::sort_keys(w.prims, w.prims_bytes, w.key_a, w.key_b, m, 0, 32 + key_bits(V), s));
    hipLaunchKernelGGL(k_low32, grid_for(m), dim3(kBlock), 0, s, w.key_b, m, w.lin_src);
    return hipGetLastError();
}

// the graph's adj_in sorted by (target, source): key_b (keys), in_pos (places in adj_in); w.in_owner filled
hipError_t sort_in_entries(const Graph& g, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL(k_owner, grid_for(g.E), dim3(kBlock), 0, s, g.in_off, g.V, g.E, w.in_owner, w.iota);
    TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pair_keys, grid_for(g.E), dim3(kBlock), 0, s, w.in_owner, g.in_nodes, g.E, w.key_a);
    TRY(hipGetLastError());
    return prims::sort_pairs(w.prims, w.prims_bytes, w.key_a, w.key_b, w.iota, w.in_pos, g.E, 0, 32 + key_bits(g.V), s);
}

// out entries in stable target order: src, tgt_orig (list order), perm (positions), tgt (sorted targets)
hipError_t target_order(const Graph& g, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL(k_owner, grid_for(g.E), dim3(kBlock), 0, s, g.out_off, g.V, g.E, w.src, w.iota);
    TRY(hipGetLastError());
    hipLaunchKernelGGL(k_out_keys, grid_for(g.E), dim3(kBlock), 0, s, g.edges, w.src, g.E, w.tgt_orig, w.key_a);
    TRY(hipGetLastError());
    TRY(prims::sort_pairs(w.prims, w.prims_bytes, w.key_a, w.key_b, w.iota, w.perm, g.E, 0, 32 + key_bits(g.V), s));
    hipLaunchKernelGGL(k_low32, grid_for(g.E), dim3(kBlock), 0, s, w.key_b, g.E, w.tgt);
    return hipGetLastError();
}

// the kept entries into `out`: records (through perm when given), seq, out_off from the sources; adj_in from in_keep
// (adj_in order kept) or, with in_keep == nullptr, rebuilt in vertex order
hipError_t emit(const Graph& in, Graph& out, const uint8_t* keep, const uint32_t* perm, const uint8_t* in_keep, const Work& w, hipStream_t s) {
    unsigned long long* d_n = w.counters + 4;
    unsigned long long* d_ni = w.counters + 5;
    TRY(prims::select_flagged(w.prims, w.prims_bytes, keep, in.E, w.idx, d_n, s));
    hipLaunchKernelGGL(k_gather_out, grid_for(in.E), dim3(kBlock), 0, s, w.idx, d_n, perm, in.edges, in.seq, out.edges, out.seq, w.lsrc[0], w.src);
    TRY(hipGetLastError());
    unsigned long long n = 0;
    TRY(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    out.V = in.V;
    out.E = (uint32_t)n;
    TRY(offsets_of(w.lsrc[0], out.E, in.V, out.out_off, w, s));
    if (in_keep) {
        TRY(prims::select_flagged(w.prims, w.prims_bytes, in_keep, in.E, w.idx, d_ni, s));
        hipLaunchKernelGGL(k_gather_u32, grid_for(in.E), dim3(kBlock), 0, s, w.idx, d_ni, in.in_nodes, out.in_nodes);
        TRY(hipGetLastError());
        hipLaunchKernelGGL(k_gather_u32, grid_for(in.E), dim3(kBlock), 0, s, w.idx, d_ni, w.in_owner, w.ltgt[0]);
        TRY(hipGetLastError());
        unsigned long long ni = 0;
        TRY(hipMemcpyAsync(&ni, d_ni, sizeof ni, hipMemcpyDeviceToHost, s));
        TRY(hipStreamSynchronize(s));
        if (ni != n) return hipErrorInvalidValue;  // adj_in and adj_out disagree
        return offsets_of(w.ltgt[0], out.E, in.V, out.in_off, w, s);
    }
    // adj_in in vertex order (:1037-1045): sources ascending in every list
    hipLaunchKernelGGL(k_owner, grid_for(out.E), dim3(kBlock), 0, s, out.out_off, in.V, out.E, w.lsrc[1], (uint32_t*)nullptr);
    TRY(hipGetLastError());
    // targets of the new records
    hipLaunchKernelGGL(k_out_keys, grid_for(out.E), dim3(kBlock), 0, s, out.edges, w.lsrc[1], out.E, w.ltgt[1], w.key_a);
    TRY(hipGetLastError());
    TRY(sorted_in_lists(w.lsrc[1], w.ltgt[1], out.E, in.V, w, s));
    TRY(hipMemcpyAsync(out.in_off, w.lin_off, ((size_t)in.V + 1) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    if (out.E) TRY(hipMemcpyAsync(out.in_nodes, w.lin_src, (size_t)out.E * 4, hipMemcpyDeviceToDevice, s));
    return hipSuccess;
}

// sortAdjOut (:806-833): stable target order (target_order), then std::sort's order in the lists where the two can differ;
// w.tied must be zero on entry
hipError_t std_sort_target_order(const Graph& g, const Work& w, uint64_t* n_tied_out, hipStream_t s) {
    // sortAdjOut: stable target order, then std::sort's order in the lists where the two can differ
    TRY(target_order(g, w, s));
    uint64_t n_tied = 0;
    const uint32_t E = g.E, V = g.V;
    if (E && V) {
        hipLaunchKernelGGL(k_tied, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, g.out_off, E, w.tied);
        TRY(hipGetLastError());
        TRY(prims::select_flagged(w.prims, w.prims_bytes, w.tied, V, w.tied_list, w.counters + 6, s));
        unsigned long long t = 0;
        TRY(hipMemcpyAsync(&t, w.counters + 6, sizeof t, hipMemcpyDeviceToHost, s));
        TRY(hipStreamSynchronize(s));
        n_tied = t;
    }
    if (n_tied) {
        // the listed lists' targets packed back to back (one copy down), std::sort's permutation of each on the host,
        // the permutations unpacked into perm (one copy up); everything on s
        std::vector<uint32_t> tied(n_tied);
        std::vector<unsigned long long> off(V + 1);
        TRY(hipMemcpyAsync(tied.data(), w.tied_list, n_tied * 4, hipMemcpyDeviceToHost, s));
        TRY(hipMemcpyAsync(off.data(), g.out_off, ((size_t)V + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        TRY(hipStreamSynchronize(s));
        std::vector<uint32_t> pack_off(n_tied + 1, 0);  // every listed list has more than 16 entries: n_tied + 1 <= E
        for (uint64_t t = 0; t < n_tied; t++) pack_off[t + 1] = pack_off[t] + (uint32_t)(off[tied[t] + 1] - off[tied[t]]);
        const uint32_t packed = pack_off[n_tied];
        uint32_t* d_pack = w.lsrc[1];      // scratch of the later passes, free here: packed <= E
        uint32_t* d_pack_off = w.ltgt[1];
        TRY(hipMemcpyAsync(d_pack_off, pack_off.data(), (n_tied + 1) * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pack_lists, dim3((unsigned)std::min<uint64_t>(n_tied, 1u << 16)), dim3(kBlock), 0, s, w.tied_list, (uint32_t)n_tied,
                           g.out_off, d_pack_off, w.tgt_orig, d_pack);
        TRY(hipGetLastError());
        std::vector<uint32_t> targets(packed), perm(packed);
        TRY(hipMemcpyAsync(targets.data(), d_pack, (size_t)packed * 4, hipMemcpyDeviceToHost, s));
        TRY(hipStreamSynchronize(s));
        for (uint64_t t = 0; t < n_tied; t++) target_sort_perm(targets.data() + pack_off[t], pack_off[t + 1] - pack_off[t], perm.data() + pack_off[t]);
        TRY(hipMemcpyAsync(d_pack, perm.data(), (size_t)packed * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_unpack_perm, dim3((unsigned)std::min<uint64_t>(n_tied, 1u << 16)), dim3(kBlock), 0, s, w.tied_list, (uint32_t)n_tied,
                           g.out_off, d_pack_off, d_pack, w.perm);
        TRY(hipGetLastError());
        TRY(hipStreamSynchronize(s));  // the host vectors leave scope
    }
    *n_tied_out = n_tied;
    return hipSuccess;
}

// ---- removeTips (:543-637) and removeBranches (:835-936) -----------------------------------------------------------
//   per-list sums       one lane per list of fewer than 64 entries, the whole wave for a longer one (a 6 000-entry hub is
//                       94 wave steps, not one lane's loop); no atomics: "has an edge that leads on" and the reduced
//                       graph's degrees are sums over a list
//   tips                one pass over the out entries in stable target order and one over the sorted in-entries, which
//                       finds the first x -> i record by binary search of the target-ordered list; a removed pair is
//                       marked at the first entry of its run (marking twice is marking once: the std::set), the marks
//                       are the removal order (ascending (v, w)), the first record of the run is the first in list order
//   branches            std::sort's target order, k_intersect on every edge, degrees of the reduced graph with
//                       multiplicity, survivors (outdeg_red(u) == 1 && indeg_red(w) == 1) united in one lock-free
//                       union-find pass (the larger root hooks under the smaller by atomicCAS, so parent[x] <= x always
//                       and a cycle's last edge finds both ends under one root), labels by one compress pass

__global__ void k_check_reads(const hc_edge_rec* __restrict__ E, uint32_t n, uint64_t n_reads, unsigned long long* __restrict__ bad) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (n + stride - 1) / stride * stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride)
        wave_count(i < n && (E[i].read1 >= n_reads || E[i].read2 >= n_reads), bad);
}

__global__ void k_count_nonzero(const uint8_t* __restrict__ a, uint32_t n, unsigned long long* __restrict__ count) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (n + stride - 1) / stride * stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) wave_count(i < n && a[i] != 0, count);
}

// out[v] = sum of f(k) over k in [off[v], off[v + 1]).  A wave takes 64 lists: lanes walk the short ones, the wave walks
// each list of 64 or more entries together.
template <class F>
__global__ void __launch_bounds__(kBlock) k_list_sum(const unsigned long long* __restrict__ off, uint32_t V, F f, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); (uint64_t)chunk * 64 < V; chunk += n_waves) {
        const uint32_t v = chunk * 64 + lane;
        const bool valid = v < V;
        const uint32_t a = valid ? (uint32_t)off[v] : 0u, b = valid ? (uint32_t)off[v + 1] : 0u;
        uint32_t sum = 0;
        if (b - a < 64)
            for (uint32_t k = a; k < b; k++) sum += f(k);
        unsigned long long longs = __ballot(b - a >= 64);
        while (longs) {
            const int j = __ffsll((long long)longs) - 1;
            longs &= longs - 1;
            const uint32_t aj = __shfl(a, j), bj = __shfl(b, j);
            uint32_t part = 0;
            for (uint32_t k = aj + lane; k < bj; k += 64) part += f(k);
            for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
            if ((int)lane == j) sum = part;
        }
        if (valid) out[v] = sum;
    }
}

struct LeadsOn {  // the entry's neighbour has a non-empty list of the same kind: the edge is no dead end
    const uint32_t* nb;
    const unsigned long long* off;
    __device__ uint32_t operator()(uint32_t k) const {
        const uint32_t t = nb[k];
        return off[t + 1] > off[t] ? 1u : 0u;
    }
};

struct KeptOut {  // target-ordered out entry k is an edge of the reduced graph
    const uint8_t* transitive;
    __device__ uint32_t operator()(uint32_t k) const { return transitive[k] ? 0u : 1u; }
};

// the first entry of (x, y)'s run in x's target-ordered out-list, or 0xffffffff
__device__ __forceinline__ uint32_t find_pair(const unsigned long long* out_off, const uint32_t* tgt, uint32_t x, uint32_t y) {
    const uint64_t o0 = out_off[x], o1 = out_off[x + 1];
    const uint32_t f = (uint32_t)o0 + lower_bound_u32(tgt + o0, (uint32_t)(o1 - o0), y);
    return f < o1 && tgt[f] == y ? f : 0xffffffffu;  // hc_graph_load checks that adj_in and adj_out hold the same pairs
}

struct KeptIn {  // sorted in-entry j (key = target << 32 | source) is an edge of the reduced graph
    const uint64_t* key;
    const unsigned long long* out_off;
    const uint32_t* tgt;
    const uint8_t* transitive;
    __device__ uint32_t operator()(uint32_t j) const {
        const uint64_t k = key[j];
        const uint32_t f = find_pair(out_off, tgt, (uint32_t)k, (uint32_t)(k >> 32));
        return f != 0xffffffffu && !transitive[f] ? 1u : 0u;
    }
};

// removeTips' first loop (:551-586) over the out entries in stable target order
__global__ void k_tips_out(const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ src,
                           const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ first, uint32_t n,
                           const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ leads, const hc_read_geom* __restrict__ reads,
                           uint32_t max_tip_len, uint8_t* __restrict__ pair_mark, uint8_t* __restrict__ tip, unsigned long long* __restrict__ tips) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (n + stride - 1) / stride * stride;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < end; p += stride) {
        bool is_tip = false;
        if (p < n) {
            const uint32_t u = src[p], t = tgt[p];
            if (out_off[u + 1] - out_off[u] > 1 && out_off[t + 1] == out_off[t]) {
                const hc_edge_rec& e = E[perm[p]];
                const unsigned int ext = edge_ext_len(e, reads[e.read1], reads[e.read2], true);
                is_tip = ext < max_tip_len || ext == 0;
                if (ext == 0 || (is_tip && leads[u] != 0)) {  // an inclusion tip always goes, another one unless all are tips
                    pair_mark[first[p]] = 1;
                    tip[e.read2] = 1;
                }
            }
        }
        wave_count(is_tip, tips);
    }
}

// ... and its second loop (:591-626) over the in-entries sorted by (target, source): the edge is the first x -> i record
__global__ void k_tips_in(const uint64_t* __restrict__ key, uint32_t n, const unsigned long long* __restrict__ in_off,
                          const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ perm,
                          const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ leads, const hc_read_geom* __restrict__ reads,
                          uint32_t max_tip_len, uint8_t* __restrict__ pair_mark, uint8_t* __restrict__ tip, unsigned long long* __restrict__ tips) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (n + stride - 1) / stride * stride;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < end; j += stride) {
        bool is_tip = false;
        if (j < n) {
            const uint64_t k = key[j];
            const uint32_t x = (uint32_t)k, i = (uint32_t)(k >> 32);
            if (in_off[i + 1] - in_off[i] > 1 && in_off[x + 1] == in_off[x]) {
                const uint32_t f = find_pair(out_off, tgt, x, i);
                if (f != 0xffffffffu) {
                    const hc_edge_rec& e = E[perm[f]];
                    const unsigned int ext = edge_ext_len(e, reads[e.read1], reads[e.read2], false);
                    is_tip = ext < max_tip_len || ext == 0;
                    if (ext == 0 || (is_tip && leads[i] != 0)) {
                        pair_mark[f] = 1;
                        tip[e.read1] = 1;
                    }
                }
            }
        }
        wave_count(is_tip, tips);
    }
}

// removeEdge for every marked pair: the first record of its run leaves adj_out (keep is in list positions) ...
__global__ void k_tips_keep_out(const uint8_t* __restrict__ pair_mark, const uint32_t* __restrict__ perm, uint32_t n, uint8_t* __restrict__ keep) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) keep[perm[p]] = pair_mark[p] ? 0 : 1;
}

// ... and the first x of adj_in[i] (the sort is stable: the first of equal keys is the first in list order)
__global__ void k_tips_keep_in(const uint64_t* __restrict__ key, const uint32_t* __restrict__ in_pos, uint32_t n,
                               const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ pair_mark,
                               uint8_t* __restrict__ in_keep) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint64_t k = key[j];
        bool del = false;
        if (j == 0 || key[j - 1] != k) {
            const uint32_t f = find_pair(out_off, tgt, (uint32_t)k, (uint32_t)(k >> 32));
            del = f != 0xffffffffu && pair_mark[f] != 0;
        }
        in_keep[in_pos[j]] = del ? 0 : 1;
    }
}

__global__ void k_gather_removed(const uint32_t* __restrict__ idx, uint32_t n, const uint32_t* __restrict__ perm, const hc_edge_rec* __restrict__ E,
                                 hc_edge_rec* __restrict__ dst) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = E[perm[idx[i]]];
}

// union-find over the vertices; parent[x] <= x throughout (the larger root hooks under the smaller)
__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ uint32_t uf_root(uint32_t* parent, uint32_t v) {  // with path halving
    uint32_t curr = uf_load(parent + v);
    if (curr != v) {
        uint32_t prev = v, next;
        while (curr > (next = uf_load(parent + curr))) {
            __atomic_store_n(parent + prev, next, __ATOMIC_RELAXED);
            prev = curr;
            curr = next;
        }
    }
    return curr;
}

__global__ void k_cc_init(uint32_t* __restrict__ parent, uint32_t V) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) parent[v] = v;
}

// every surviving edge of the reduced graph unites its ends.  A failed atomicCAS returns a smaller id to go on from, so
// every retry descends and the loop ends; the edge that closes a cycle finds one root on both sides and does nothing.
__global__ void k_cc_hook(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ transitive, uint32_t n,
                          const uint32_t* __restrict__ dout, const uint32_t* __restrict__ din, uint32_t* parent) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const uint32_t u = src[p], w = tgt[p];
        if (transitive[p] || dout[u] != 1 || din[w] != 1) continue;
        uint32_t a = uf_root(parent, u), b = uf_root(parent, w);
        while (a != b) {
            if (a < b) {
                const uint32_t t = a;
                a = b;
                b = t;
            }
            const uint32_t old = atomicCAS(parent + a, a, b);  // a > b: hook a under b if a is still a root
            if (old == a) break;
            a = old;
        }
    }
}

__global__ void k_cc_labels(const uint32_t* __restrict__ parent, uint32_t V, uint32_t* __restrict__ label, unsigned long long* __restrict__ n_roots) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (V + stride - 1) / stride * stride;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < end; v += stride) {
        bool root = false;
        if (v < V) {
            uint32_t r = v, nx;
            while ((nx = parent[r]) != r) r = nx;
            label[v] = r;
            root = r == v;
        }
        wave_count(root, n_roots);
    }
}

__global__ void k_branch_stats(const uint32_t* __restrict__ dout, const uint32_t* __restrict__ din, uint32_t V, unsigned long long* __restrict__ n_out,
                               unsigned long long* __restrict__ n_in) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t end = (V + stride - 1) / stride * stride;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < end; v += stride) {
        wave_count(v < V && dout[v] > 1, n_out);
        wave_count(v < V && din[v] > 1, n_in);
    }
}

// :918-931: every record between two components leaves (target-ordered positions), and every such entry of adj_in
__global__ void k_branch_keep(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ in_owner,
                              const uint32_t* __restrict__ in_nodes, const uint32_t* __restrict__ label, uint32_t n, uint8_t* __restrict__ keep,
                              uint8_t* __restrict__ del, uint8_t* __restrict__ in_keep) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const bool same = label[src[p]] == label[tgt[p]];
        keep[p] = same ? 1 : 0;
        del[p] = same ? 0 : 1;
        in_keep[p] = label[in_nodes[p]] == label[in_owner[p]] ? 1 : 0;
    }
}

}  // namespace

hipError_t check_graph(const Graph& g, bool* consistent, void* temp, size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_) return hipErrorInvalidValue;
    *consistent = true;
    if (!g.E) return hipSuccess;
    TRY(hipMemsetAsync(w.counters, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_owner, grid_for(g.E), dim3(kBlock), 0, s, g.out_off, g.V, g.E, w.src, g.seq);  // seq = 0, 1, ...
    hipLaunchKernelGGL(k_check_ids, grid_for(g.E), dim3(kBlock), 0, s, g.edges, w.src, g.in_nodes, g.E, g.V, w.counters);
    hipLaunchKernelGGL(k_out_keys, grid_for(g.E), dim3(kBlock), 0, s, g.edges, w.src, g.E, w.tgt_orig, w.key_a);
    TRY(hipGetLastError());
    TRY(prims::sort_keys(w.prims, w.prims_bytes, w.key_a, w.key_b, g.E, 0, 64, s));  // ids not checked yet: all 64 bits
    hipLaunchKernelGGL(k_owner, grid_for(g.E), dim3(kBlock), 0, s, g.in_off, g.V, g.E, w.in_owner, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_pair_keys, grid_for(g.E), dim3(kBlock), 0, s, g.in_nodes, w.in_owner, g.E, w.key_a);
    TRY(hipGetLastError());
    TRY(prims::sort_keys(w.prims, w.prims_bytes, w.key_a, w.key_c, g.E, 0, 64, s));
    hipLaunchKernelGGL(k_compare_keys, grid_for(g.E), dim3(kBlock), 0, s, w.key_b, w.key_c, g.E, w.counters);
    TRY(hipGetLastError());
    unsigned long long bad = 0;
    TRY(hipMemcpyAsync(&bad, w.counters, sizeof bad, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    *consistent = bad == 0;
    return hipSuccess;
}

size_t temp_bytes(uint64_t E, uint64_t V) {
    Carve c{nullptr};
    layout(c, E, V);
    return c.used + 256;
}

hipError_t remove_transitive(const Graph& g, Graph& out, uint32_t remove_trans, uint32_t branch_reduction, hc_clean_counts* counts, void* temp,
                             size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_) return hipErrorInvalidValue;
    const uint32_t E = g.E, V = g.V;
    TRY(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), s));
    TRY(hipMemsetAsync(w.tied, 0, (size_t)V + 1, s));
    uint64_t n_tied = 0;
    TRY(std_sort_target_order(g, w, &n_tied, s));
    // sortAdjLists(adj_in) and the transitive passes (:954-966); level 0 = every edge in target order
    TRY(sort_in_entries(g, w, s));
    TRY(hipMemsetAsync(w.in_t, 0, E ? E : 1, s));
    TRY(hipMemsetAsync(w.in_d, 0, E ? E : 1, s));
    TRY(hipMemsetAsync(w.pair_d, 0, E ? E : 1, s));
    const uint32_t* lsrc = w.src;
    const uint32_t* ltgt = w.tgt;
    const uint32_t* lpos = nullptr;
    const unsigned long long* lout = g.out_off;
    const unsigned long long* lin = g.in_off;
    hipLaunchKernelGGL(k_low32, grid_for(E), dim3(kBlock), 0, s, w.key_b, E, w.lin_src);
    TRY(hipGetLastError());
    const uint32_t* lin_src = w.lin_src;
    uint32_t m = E;
    for (uint32_t pass = 0; pass < remove_trans && m; pass++) {
        if (pass) {
            TRY(offsets_of(lsrc, m, V, w.lout_off, w, s));
            TRY(sorted_in_lists(lsrc, ltgt, m, V, w, s));
            lout = w.lout_off;
            lin = w.lin_off;
            lin_src = w.lin_src;
        }
        hipLaunchKernelGGL(k_intersect, grid_for(m), dim3(kBlock), 0, s, lsrc, ltgt, m, lout, ltgt, lin, lin_src, w.flags);
        TRY(hipGetLastError());
        const int b = pass & 1;
        TRY(prims::select_flagged(w.prims, w.prims_bytes, w.flags, m, w.idx, w.counters + 7, s));
        hipLaunchKernelGGL(k_gather_level, grid_for(m), dim3(kBlock), 0, s, w.idx, w.counters + 7, lsrc, ltgt, lpos, w.lsrc[b], w.ltgt[b],
                           w.lpos[b]);
        TRY(hipGetLastError());
        unsigned long long k = 0;
        TRY(hipMemcpyAsync(&k, w.counters + 7, sizeof k, hipMemcpyDeviceToHost, s));
        TRY(hipStreamSynchronize(s));
        m = (uint32_t)k;
        lsrc = w.lsrc[b];
        ltgt = w.ltgt[b];
        lpos = w.lpos[b];
    }
    const uint32_t transitive = m;
    if (transitive) {
        hipLaunchKernelGGL(k_mark, grid_for(transitive), dim3(kBlock), 0, s, lpos, transitive, w.in_t);
        TRY(hipGetLastError());
    }
    if (E) {
        hipLaunchKernelGGL(k_first, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, g.out_off, E, w.first);
        TRY(hipGetLastError());
    }
    if (remove_trans == 1 && branch_reduction && transitive) {
        hipLaunchKernelGGL(k_fill_int, grid_for(2 * (V + 1)), dim3(kBlock), 0, s, w.max_out, V + 1, INT_MIN);
        hipLaunchKernelGGL(k_fill_int, grid_for(2 * (V + 1)), dim3(kBlock), 0, s, w.max_in, V + 1, INT_MIN);
        hipLaunchKernelGGL(k_branch_max, grid_for(transitive), dim3(kBlock), 0, s, lpos, transitive, w.src, w.tgt, w.first, w.perm, g.edges, w.max_out,
                           w.max_in);
        hipLaunchKernelGGL(k_branch_pairs, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, w.first, w.perm, g.edges, E, w.max_out, w.max_in, w.pair_d);
        hipLaunchKernelGGL(k_spread_pairs, grid_for(E), dim3(kBlock), 0, s, w.first, w.pair_d, E, w.in_d);
        TRY(hipGetLastError());
    }
    const bool rebuild = 1.0 * transitive > 0.5 * E;
    {
        hipLaunchKernelGGL(k_keep_out, grid_for(E), dim3(kBlock), 0, s, w.in_t, w.in_d, w.first, E, rebuild ? 1u : 0u, w.keep, w.counters + 0);
        TRY(hipGetLastError());
        if (!rebuild && E) {
            if (remove_trans > 1) TRY(sort_in_entries(g, w, s));  // the later passes used the key buffers
            hipLaunchKernelGGL(k_keep_in_removed, grid_for(E), dim3(kBlock), 0, s, w.key_b, w.in_pos, E, g.in_off, g.out_off, w.tgt, w.in_t, w.in_d, w.in_keep);
            TRY(hipGetLastError());
        }
        TRY(emit(g, out, w.keep, w.perm, rebuild ? nullptr : w.in_keep, w, s));
    }
    unsigned long long deleted = 0;
    TRY(hipMemcpyAsync(&deleted, w.counters + 0, sizeof deleted, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    counts->edges_before = E;
    counts->edges_after = out.E;
    counts->transitive_count = transitive;
    counts->del_count = deleted;
    counts->rebuilt = rebuild ? 1 : 0;
    counts->n_tied_lists = n_tied;
    if ((uint64_t)E - transitive - deleted != out.E) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t remove_inclusions(const Graph& g, const uint8_t* incl, Graph& out, uint32_t* group_vertex, unsigned long long* group_off,
                             hc_edge_rec* group_edges, uint64_t* n_groups, uint64_t* n_group_edges, hc_clean_counts* counts, void* temp,
                             size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_) return hipErrorInvalidValue;
    const uint32_t E = g.E, V = g.V;
    TRY(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), s));
    TRY(target_order(g, w, s));  // stable: the first entry of a target's run is the first in list order
    TRY(sort_in_entries(g, w, s));
    // groups: sizes, scan, the marked vertices in order
    hipLaunchKernelGGL(k_group_sizes, grid_for(V + 1), dim3(kBlock), 0, s, incl, g.out_off, g.in_off, V, w.hist);
    TRY(hipGetLastError());
    TRY(prims::exclusive_sum(w.prims, w.prims_bytes, (const uint64_t*)w.hist, (uint64_t*)w.lout_off, (uint64_t)V + 1, s));
    TRY(prims::select_flagged(w.prims, w.prims_bytes, incl, V, group_vertex, w.counters + 6, s));
    hipLaunchKernelGGL(k_group_off, grid_for(V + 1), dim3(kBlock), 0, s, group_vertex, w.counters + 6, w.lout_off, V, group_off);
    TRY(hipGetLastError());
    if (E) {
        hipLaunchKernelGGL(k_incl_out, grid_for(E), dim3(kBlock), 0, s, g.edges, w.src, w.tgt_orig, E, incl, g.out_off, w.lout_off, group_edges);
        hipLaunchKernelGGL(k_incl_keep_out, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, w.perm, g.out_off, E, incl, w.keep, w.counters + 0);
        hipLaunchKernelGGL(k_incl_in, grid_for(E), dim3(kBlock), 0, s, w.key_b, w.in_pos, E, g.in_off, g.out_off, w.tgt, w.perm, g.edges, incl,
                           w.lout_off, group_edges, w.in_keep);
        TRY(hipGetLastError());
    }
    // src in list order for emit (target_order left it per position, which is the same vertex)
    TRY(emit(g, out, w.keep, nullptr, w.in_keep, w, s));
    unsigned long long h[8];
    unsigned long long total = 0;
    TRY(hipMemcpyAsync(h, w.counters, sizeof h, hipMemcpyDeviceToHost, s));
    TRY(hipMemcpyAsync(&total, w.lout_off + V, sizeof total, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    *n_groups = h[6];
    *n_group_edges = total;
    counts->edges_before = E;
    counts->edges_after = out.E;
    counts->transitive_count = 0;
    counts->del_count = h[0];
    counts->rebuilt = 0;
    counts->n_tied_lists = 0;
    if ((uint64_t)E - h[0] != out.E) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t find_tips(const Graph& g, uint32_t max_tip_len, const hc_read_geom* reads, uint64_t n_reads, uint8_t* tip, uint64_t n_flags, hc_tip_counts* counts,
                     bool* reads_in_range, void* temp, size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_ || !g.E) return hipErrorInvalidValue;
    const uint32_t E = g.E, V = g.V;
    TRY(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_check_reads, grid_for(E), dim3(kBlock), 0, s, g.edges, E, n_reads, w.counters + 2);
    TRY(hipGetLastError());
    unsigned long long bad = 0;
    TRY(hipMemcpyAsync(&bad, w.counters + 2, sizeof bad, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    *reads_in_range = bad == 0;
    if (bad) return hipSuccess;
    TRY(target_order(g, w, s));  // stable: the first entry of a target's run is the first in list order
    TRY(sort_in_entries(g, w, s));
    TRY(hipMemsetAsync(w.pair_d, 0, E, s));
    uint32_t* leads_out = (uint32_t*)w.max_out;
    uint32_t* leads_in = (uint32_t*)w.max_in;
    const dim3 vgrid = grid_for(((uint64_t)V + 63) / 64 * 64);  // 64 lists per wave
    hipLaunchKernelGGL(k_first, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, g.out_off, E, w.first);
    hipLaunchKernelGGL(k_list_sum<LeadsOn>, vgrid, dim3(kBlock), 0, s, g.out_off, V, LeadsOn{w.tgt_orig, g.out_off}, leads_out);
    hipLaunchKernelGGL(k_list_sum<LeadsOn>, vgrid, dim3(kBlock), 0, s, g.in_off, V, LeadsOn{g.in_nodes, g.in_off}, leads_in);
    hipLaunchKernelGGL(k_tips_out, grid_for(E), dim3(kBlock), 0, s, g.edges, w.perm, w.src, w.tgt, w.first, E, g.out_off, leads_out, reads,
                       max_tip_len, w.pair_d, tip, w.counters + 0);
    hipLaunchKernelGGL(k_tips_in, grid_for(E), dim3(kBlock), 0, s, w.key_b, E, g.in_off, g.out_off, w.tgt, w.perm, g.edges, leads_in, reads,
                       max_tip_len, w.pair_d, tip, w.counters + 1);
    hipLaunchKernelGGL(k_tips_keep_out, grid_for(E), dim3(kBlock), 0, s, w.pair_d, w.perm, E, w.keep);
    hipLaunchKernelGGL(k_tips_keep_in, grid_for(E), dim3(kBlock), 0, s, w.key_b, w.in_pos, E, g.out_off, w.tgt, w.pair_d, w.in_keep);
    hipLaunchKernelGGL(k_count_nonzero, grid_for(n_flags), dim3(kBlock), 0, s, tip, (uint32_t)n_flags, w.counters + 7);
    TRY(hipGetLastError());
    TRY(prims::select_flagged(w.prims, w.prims_bytes, w.pair_d, E, w.lpos[1], w.counters + 3, s));  // ascending (v, w)
    unsigned long long h[8];
    TRY(hipMemcpyAsync(h, w.counters, sizeof h, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    counts->edges_before = E;
    counts->out_tip_count = h[0];
    counts->tip_count = h[0] + h[1];
    counts->n_removed = h[3];
    counts->n_tip_reads = h[7];
    return hipSuccess;
}

hipError_t find_branches(const Graph& g, hc_branch_counts* counts, void* temp, size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_ || !g.E) return hipErrorInvalidValue;
    const uint32_t E = g.E, V = g.V;
    TRY(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), s));
    TRY(hipMemsetAsync(w.tied, 0, (size_t)V + 1, s));
    uint64_t n_tied = 0;
    TRY(std_sort_target_order(g, w, &n_tied, s));  // sortAdjOut; sortAdjLists(adj_in) next
    TRY(sort_in_entries(g, w, s));
    hipLaunchKernelGGL(k_low32, grid_for(E), dim3(kBlock), 0, s, w.key_b, E, w.lin_src);
    // findTransEdges(..., removeTrans = true) (:847): the reduced graph is what the intersection test does not flag
    hipLaunchKernelGGL(k_intersect, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, E, g.out_off, w.tgt, g.in_off, w.lin_src, w.flags);
    TRY(hipGetLastError());
    uint32_t* dout = (uint32_t*)w.max_out;
    uint32_t* din = (uint32_t*)w.max_in;
    uint32_t* parent = w.tied_list;     // free once the target order stands
    uint32_t* label = (uint32_t*)w.hist;
    const dim3 vgrid = grid_for(((uint64_t)V + 63) / 64 * 64);
    hipLaunchKernelGGL(k_list_sum<KeptOut>, vgrid, dim3(kBlock), 0, s, g.out_off, V, KeptOut{w.flags}, dout);
    hipLaunchKernelGGL(k_list_sum<KeptIn>, vgrid, dim3(kBlock), 0, s, g.in_off, V, KeptIn{w.key_b, g.out_off, w.tgt, w.flags}, din);
    hipLaunchKernelGGL(k_count_nonzero, grid_for(E), dim3(kBlock), 0, s, w.flags, E, w.counters + 0);
    hipLaunchKernelGGL(k_branch_stats, grid_for(V), dim3(kBlock), 0, s, dout, din, V, w.counters + 1, w.counters + 2);
    // components of the surviving edges over all V vertices: one hooking pass, one compress pass
    hipLaunchKernelGGL(k_cc_init, grid_for(V), dim3(kBlock), 0, s, parent, V);
    hipLaunchKernelGGL(k_cc_hook, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, w.flags, E, dout, din, parent);
    hipLaunchKernelGGL(k_cc_labels, grid_for(V), dim3(kBlock), 0, s, parent, V, label, w.counters + 7);
    hipLaunchKernelGGL(k_branch_keep, grid_for(E), dim3(kBlock), 0, s, w.src, w.tgt, w.in_owner, g.in_nodes, label, E, w.keep, w.in_d, w.in_keep);
    TRY(hipGetLastError());
    TRY(prims::select_flagged(w.prims, w.prims_bytes, w.in_d, E, w.lpos[1], w.counters + 3, s));  // vertex ascending, list order
    unsigned long long h[8];
    TRY(hipMemcpyAsync(h, w.counters, sizeof h, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    counts->edges_before = E;
    counts->transitive_kept = E - h[0];
    counts->n_out_branch = h[1];
    counts->n_in_branch = h[2];
    counts->n_removed = h[3];
    counts->n_components = h[7];
    counts->n_tied_lists = n_tied;
    counts->cc_rounds = 0;
    return hipSuccess;
}

hipError_t commit_removed(const Graph& g, Graph& out, bool target_ordered, hc_edge_rec* removed, uint64_t n_removed, void* temp, size_t temp_bytes_,
                          hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_ || n_removed > g.E) return hipErrorInvalidValue;
    if (n_removed) {
        hipLaunchKernelGGL(k_gather_removed, grid_for(n_removed), dim3(kBlock), 0, s, w.lpos[1], (uint32_t)n_removed, w.perm, g.edges, removed);
        TRY(hipGetLastError());
    }
    TRY(emit(g, out, w.keep, target_ordered ? w.perm : nullptr, w.in_keep, w, s));
    if ((uint64_t)g.E - n_removed != out.E) return hipErrorInvalidValue;
    return hipSuccess;
}

__global__ void k_drop_listed(const uint32_t* __restrict__ rec, const uint32_t* __restrict__ in_pos, uint32_t n, const hc_edge_rec* __restrict__ E,
                              uint8_t* __restrict__ keep, uint8_t* __restrict__ in_keep, hc_edge_rec* __restrict__ removed) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        keep[rec[i]] = 0;
        in_keep[in_pos[i]] = 0;
        removed[i] = E[rec[i]];
    }
}

hipError_t remove_records(const Graph& g, Graph& out, const uint32_t* rec, const uint32_t* in_pos, uint32_t n, hc_edge_rec* removed, void* temp,
                          size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_ || !g.E || n > g.E) return hipErrorInvalidValue;
    TRY(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), s));
    TRY(hipMemsetAsync(w.keep, 1, g.E, s));
    TRY(hipMemsetAsync(w.in_keep, 1, g.E, s));
    hipLaunchKernelGGL(k_owner, grid_for(g.E), dim3(kBlock), 0, s, g.out_off, g.V, g.E, w.src, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_owner, grid_for(g.E), dim3(kBlock), 0, s, g.in_off, g.V, g.E, w.in_owner, (uint32_t*)nullptr);
    if (n) hipLaunchKernelGGL(k_drop_listed, grid_for(n), dim3(kBlock), 0, s, rec, in_pos, n, g.edges, w.keep, w.in_keep, removed);
    TRY(hipGetLastError());
    TRY(emit(g, out, w.keep, nullptr, w.in_keep, w, s));
    if ((uint64_t)g.E - n != out.E) return hipErrorInvalidValue;
    return hipSuccess;
}

__global__ void k_permute_records(const uint32_t* __restrict__ perm, uint32_t n, const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ seq,
                                  hc_edge_rec* __restrict__ E_out, uint32_t* __restrict__ seq_out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t k = perm[i];
        E_out[i] = E[k];
        seq_out[i] = seq[k];
    }
}

hipError_t sort_adj_out(const Graph& g, Graph& out, uint64_t* n_tied_lists, void* temp, size_t temp_bytes_, hipStream_t s) {
    Carve c{(char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255)};
    const Work w = layout(c, g.E, g.V);
    if (c.used + 256 > temp_bytes_ || !g.E) return hipErrorInvalidValue;
    TRY(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), s));
    TRY(hipMemsetAsync(w.tied, 0, (size_t)g.V + 1, s));
    TRY(std_sort_target_order(g, w, n_tied_lists, s));
    hipLaunchKernelGGL(k_permute_records, grid_for(g.E), dim3(kBlock), 0, s, w.perm, g.E, g.edges, g.seq, out.edges, out.seq);
    return hipGetLastError();
}

}  // namespace trans
}  // namespace hc
