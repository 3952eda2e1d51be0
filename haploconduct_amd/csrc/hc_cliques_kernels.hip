// hc_cliques_kernels.hip — the device side of hc_graph_cliques (include/hcedge.h): every maximal clique of the graph
// OverlapGraph::writeGraphToFile describes (reference src/OverlapGraph.cpp:322-385), in the order of host/CliqueRule.h.  A fixed number
// of launches whatever the graph:
//
// emit_pairs_kernel (a lane per out-record) writes the record's pair both ways as packed keys, or the skip key for an inclusion
//   endpoint, and does the reference's two asserts: one atomicMin per workgroup on the packed place (hc_graph_text.h) leaves the first
//   in file order.  One radix sort and hc::prims::unique make the pair set; offsets_kernel (a lane per vertex, a binary search) and
//   neighbours_kernel cut it into the simple adjacency, lists ascending; one more sort of (degree, id) gives the rank.
// classify_kernel (a lane per root) counts the neighbours of greater rank: a root without any is settled here (degree 0: its own
//   clique; otherwise nothing), the others are a wave's or, above root_cap, the host's.
// bk_kernel<WRITE> (a wave per root, roots by ticket from the heaviest rank down).  The wave builds the d x ceil(d / 64)-word bit
//   matrix of N(v)'s induced subgraph in its own scratch slice, a lane per row, and walks Bron-Kerbosch with pivoting iteratively:
//   level l of the stack holds P, X and the candidates left.  Pivot scoring is the hot loop: a lane per member of P | X, popcount of
//   row & P over the words, a wave max over the packed key (score, smallest index).  Set updates are lanes over words.  The count
//   form adds up cliques and entries per root, tests the budget inside a root and, per wave, every 32 roots; the write form repeats the walk and
//   puts each clique at its place — the members in ascending id by a walk over R's bits, the root inserted — with no output atomics.
// Scratch is per resident wave, never per root.  The wave's lanes meet through that scratch: every group of stores is followed by a
// wavefront-scope fence before another lane reads it.  Plain HIP C++, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_cliques.h"
#include "hc_graph_text.h"

namespace hc {
namespace cliques {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kFlushRoots = 32;  // roots a wave counts before it adds its entries to the budget counter

__device__ __forceinline__ void wave_sync() {  // what the wave's lanes stored is what its lanes load from here on
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kBlock) void emit_pairs_kernel(Graph g, uint32_t shift, uint64_t* __restrict__ keys,
                                                            unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long first_bad;
    if (threadIdx.x == 0) first_bad = gtext::kNoKey;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < g.n_edges) {
        const uint32_t i = (uint32_t)g.E[k].v1, j = (uint32_t)g.E[k].v2;
        const uint64_t skip = 1ull << (2u * shift);
        uint64_t a = skip, b = skip, bad = gtext::kNoKey;
        if (g.incl[i]) bad = gtext::bad_key(i, 0, 1);  // :346, a status of the vertex
        else if (g.incl[j]) {                          // :352
        } else if (j == i) bad = gtext::bad_key(i, (uint32_t)(k - g.out_off[i]) + 1u, 0);  // :355
        else a = (uint64_t)i << shift | j, b = (uint64_t)j << shift | i;
        keys[2 * k] = a;
        keys[2 * k + 1] = b;
        if (bad != gtext::kNoKey) atomicMin(&first_bad, (unsigned long long)bad);
    }
    __syncthreads();
    if (threadIdx.x == 0 && first_bad != gtext::kNoKey) atomicMin(&counters[kKey], first_bad);
}

// off[v] = the first distinct key >= v << shift, v = 0 .. V (V << shift <= the skip key)
__global__ __launch_bounds__(kBlock) void offsets_kernel(const uint64_t* __restrict__ uniq, uint32_t shift, Adj a,
                                                         const unsigned long long* __restrict__ counters) {
    const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v > a.V) return;
    const uint64_t t = v << shift;
    uint64_t lo = 0, hi = counters[kUnique];
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (uniq[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    a.off[v] = lo;
}

__global__ __launch_bounds__(kBlock) void neighbours_kernel(const uint64_t* __restrict__ uniq, uint64_t n_keys, uint32_t shift, Adj a,
                                                            uint64_t* __restrict__ rank_keys, unsigned long long* __restrict__ counters) {
    __shared__ unsigned int max_deg;
    if (threadIdx.x == 0) max_deg = 0;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n_keys && k < a.off[a.V]) a.nbr[k] = (uint32_t)(uniq[k] & ((1ull << shift) - 1));
    if (k < a.V) {
        const uint32_t d = (uint32_t)(a.off[k + 1] - a.off[k]);
        rank_keys[k] = rank_key(d, (uint32_t)k);
        atomicMax(&max_deg, d);
    }
    __syncthreads();
    if (threadIdx.x == 0 && max_deg) atomicMax(&counters[kMaxDeg], (unsigned long long)max_deg);
}

__global__ __launch_bounds__(kBlock) void rank_kernel(const uint64_t* __restrict__ sorted, Adj a) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.V) return;
    const uint32_t v = (uint32_t)sorted[r];
    a.order[r] = v;
    a.rank[v] = (uint32_t)r;
}

__global__ __launch_bounds__(kBlock) void classify_kernel(Adj a, uint64_t* __restrict__ cnt_c, uint64_t* __restrict__ cnt_e,
                                                          unsigned long long* __restrict__ counters) {
    __shared__ unsigned int tally[2];  // host roots, singletons
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r <= a.V) cnt_c[r] = 0, cnt_e[r] = 0;
    if (r < a.V) {
        const uint32_t v = a.order[r];
        const uint64_t b = a.off[v], e = a.off[v + 1];
        bool any_P = false;
        for (uint64_t k = b; k < e && !any_P; k++) any_P = starts_in_P(a.rank[a.nbr[k]], (uint32_t)r);
        uint8_t kind = kRootTrivial;
        if (e == b) {  // P = {} and X = {}: {v}
            cnt_c[r] = 1, cnt_e[r] = 1;
            atomicAdd(&tally[1], 1u);
        } else if (any_P) {
            kind = e - b <= a.cap ? kRootDevice : kRootHost;
            if (kind == kRootHost) atomicAdd(&tally[0], 1u);
        }
        a.kind[r] = kind;
    }
    __syncthreads();
    if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(&counters[threadIdx.x == 0 ? kHostRoots : kSingletons], (unsigned long long)tally[threadIdx.x]);
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
    for (int o = 32; o; o >>= 1) {
        const uint64_t w = (uint64_t)__shfl_xor((long long)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

template <bool WRITE>
__global__ __launch_bounds__(kBlock) void bk_kernel(Adj g, uint64_t* __restrict__ cnt_c, uint64_t* __restrict__ cnt_e, uint64_t* __restrict__ scratch,
                                                    uint32_t dmax, uint64_t budget, unsigned long long* __restrict__ counters,
                                                    unsigned long long* __restrict__ clique_off, uint32_t* __restrict__ clique_nodes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint32_t Wm = words_of(dmax);
    uint64_t* const M = scratch + wave * slice_words(dmax);
    uint64_t* const ST = M + (uint64_t)dmax * Wm;
    uint64_t* const R = ST + ((uint64_t)dmax + 1) * 3 * Wm;
    uint32_t* const cur = (uint32_t*)(R + Wm);
    uint64_t pend_e = 0;  // count pass: the wave's entries since its last flush to the budget counter, over pend_n roots
    uint32_t pend_n = 0, wave_biggest = 0;
    for (;;) {
        unsigned long long t = 0;
        int stop = 0;
        if (lane == 0) {
            t = atomicAdd(&counters[kTicket], 1ull);
            stop = !WRITE && __hip_atomic_load(&counters[kOver], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        }
        t = (unsigned long long)__shfl((long long)t, 0, 64);
        if (t >= g.V || __shfl(stop, 0, 64)) break;  // (lane 0's view for the whole wave)
        const uint32_t r = g.V - 1u - (uint32_t)t;  // the heaviest first
        if (g.kind[r] != kRootDevice) continue;
        const uint32_t v = g.order[r];
        const uint32_t* __restrict__ N = g.nbr + g.off[v];
        const uint32_t d = (uint32_t)(g.off[v + 1] - g.off[v]);  // 1 <= d <= min(cap, the largest degree) = dmax
        const uint32_t W = words_of(d);
        // level 0: P = the neighbours of greater rank, X = the others; R = {}; lt = the neighbours below v
        uint32_t lt = 0;
        for (uint32_t base = 0; base < d; base += 64) {
            const uint32_t a = base + lane;
            const bool in = a < d;
            const uint32_t u = in ? N[a] : 0u;
            const unsigned long long all = __ballot(in), p = __ballot(in && starts_in_P(g.rank[u], r));
            lt += (uint32_t)__popcll(__ballot(in && u < v));
            if (lane == 0) {
                ST[base >> 6] = p;
                ST[W + (base >> 6)] = all & ~p;
                R[base >> 6] = 0;
            }
        }
        for (uint32_t a = lane; a < d; a += 64) {
            const uint32_t u = N[a];
            matrix_row(g.nbr + g.off[u], (uint32_t)(g.off[u + 1] - g.off[u]), N, d, M + (uint64_t)a * W);
        }
        wave_sync();
        uint64_t nc = 0, ne = 0;
        uint32_t level = 0, biggest = 0;
        bool entering = true, over = false;
        const uint64_t c0 = WRITE ? cnt_c[r] : 0, e0 = WRITE ? cnt_e[r] : 0;
        for (;;) {
            uint64_t* const P = ST + (uint64_t)level * 3 * W;
            uint64_t* const X = P + W;
            uint64_t* const C = X + W;
            bool pop = false;
            if (entering) {
                uint64_t accP = 0, accX = 0;
                for (uint32_t w = lane; w < W; w += 64) accP |= P[w], accX |= X[w];
                const bool any_P = __ballot(accP != 0) != 0, any_X = __ballot(accX != 0) != 0;
                if (!any_P) {
                    if (emits(any_P, any_X)) {  // R and the root: level + 1 vertices
                        if (WRITE) {
                            const uint64_t at = e0 + ne;
                            uint32_t before = 0;  // members of R in the words behind
                            for (uint32_t w = 0; w < W; w++) {
                                const uint64_t word = R[w];
                                const uint32_t b = w * 64 + lane;
                                if (word >> lane & 1ull) {
                                    const uint32_t q = before + (uint32_t)__popcll(word & ((1ull << lane) - 1));
                                    clique_nodes[at + q + (b >= lt ? 1u : 0u)] = N[b];
                                }
                                if (lane == 0 && w == (lt >> 6)) clique_nodes[at + before + (uint32_t)__popcll(word & ((1ull << (lt & 63u)) - 1))] = v;
                                before += (uint32_t)__popcll(word);
                            }
                            if (lane == 0) {
                                if (W == (lt >> 6)) clique_nodes[at + before] = v;  // (lt = d = 64 * W: the root is the last)
                                clique_off[c0 + nc] = at;
                            }
                        }
                        nc++;
                        ne += level + 1;
                        biggest = level + 1 > biggest ? level + 1 : biggest;
                        if (!WRITE && ne > budget) {
                            over = true;
                            break;
                        }
                    }
                    pop = true;
                } else {
                    uint64_t best = 0;
                    for (uint32_t w = 0; w < W; w++) {
                        const uint64_t both = P[w] | X[w];
                        if (both >> lane & 1ull) {
                            const uint32_t u = w * 64 + lane;
                            const uint64_t* __restrict__ row = M + (uint64_t)u * W;
                            uint32_t score = 0;
                            for (uint32_t w2 = 0; w2 < W; w2++) score += (uint32_t)__popcll(row[w2] & P[w2]);
                            const uint64_t key = pivot_key(score, u);
                            best = key > best ? key : best;
                        }
                    }
                    const uint64_t* __restrict__ prow = M + (uint64_t)pivot_of(wave_max(best)) * W;
                    for (uint32_t w = lane; w < W; w += 64) C[w] = candidates(P[w], prow[w]);
                    wave_sync();
                }
                entering = false;
            }
            if (!pop) {  // the next candidate: the lowest bit left
                uint32_t w = 0;
                uint64_t cw = 0;
                for (; w < W; w++)
                    if ((cw = C[w]) != 0) break;
                if (w == W) {
                    pop = true;
                } else {
                    const uint32_t b = w * 64 + (uint32_t)__builtin_ctzll(cw);
                    const uint64_t* __restrict__ row = M + (uint64_t)b * W;
                    uint64_t* const P1 = P + 3 * (uint64_t)W;
                    for (uint32_t w2 = lane; w2 < W; w2 += 64) P1[w2] = P[w2] & row[w2], P1[W + w2] = X[w2] & row[w2];
                    wave_sync();  // (lane 0 changes C[w] and R only after every lane has read them)
                    if (lane == 0) {
                        C[w] = cw & (cw - 1);
                        cur[level] = b;
                        R[b >> 6] |= 1ull << (b & 63u);
                    }
                    wave_sync();
                    level++;
                    entering = true;
                    continue;
                }
            }
            if (level == 0) break;  // pop: the vertex the level below took moves from P to X
            level--;
            const uint32_t b = cur[level];
            wave_sync();
            if (lane == 0) {
                uint64_t* const P0 = ST + (uint64_t)level * 3 * W;
                const uint64_t bit = 1ull << (b & 63u);
                R[b >> 6] &= ~bit;
                P0[b >> 6] &= ~bit;
                P0[W + (b >> 6)] |= bit;
            }
            wave_sync();
        }
        if (!WRITE) {
            if (lane == 0) cnt_c[r] = nc, cnt_e[r] = ne;
            pend_e += ne;
            pend_n++;
            wave_biggest = biggest > wave_biggest ? biggest : wave_biggest;
            // one atomic on the budget counter per kFlushRoots roots, not per root (the same address for every wave), and at once
            // where the wave alone is sure
            if (over || pend_n == kFlushRoots || pend_e > budget) {
                if (lane == 0) {
                    const unsigned long long total = atomicAdd(&counters[kTotal], (unsigned long long)pend_e) + pend_e;
                    if (over || total > budget) atomicExch(&counters[kOver], 1ull);
                }
                pend_e = 0, pend_n = 0;
            }
        }
        wave_sync();  // (the next root's level 0 overwrites what lanes may still be reading)
        if (over) break;
    }
    if (!WRITE && lane == 0) {
        if (pend_e) {
            const unsigned long long total = atomicAdd(&counters[kTotal], (unsigned long long)pend_e) + pend_e;
            if (total > budget) atomicExch(&counters[kOver], 1ull);
        }
        if (wave_biggest) atomicMax(&counters[kMaxClique], (unsigned long long)wave_biggest);
    }
}

// the trivial roots' cliques ({v} for a vertex without pairs) and the end of clique_off
__global__ __launch_bounds__(kBlock) void write_trivial_kernel(Adj a, const uint64_t* __restrict__ cnt_c, const uint64_t* __restrict__ cnt_e,
                                                               unsigned long long* __restrict__ clique_off, uint32_t* __restrict__ clique_nodes) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r == a.V) clique_off[cnt_c[r]] = cnt_e[r];
    if (r >= a.V || a.kind[r] != kRootTrivial || cnt_c[r + 1] == cnt_c[r]) return;
    clique_off[cnt_c[r]] = cnt_e[r];
    clique_nodes[cnt_e[r]] = a.order[r];
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t emit_pairs(const Graph& g, uint32_t shift, uint64_t* keys, unsigned long long* counters, hipStream_t s) {
    if (g.n_edges) hipLaunchKernelGGL(emit_pairs_kernel, dim3(blocks_for(g.n_edges)), dim3(kBlock), 0, s, g, shift, keys, counters);
    return hipGetLastError();
}

hipError_t build_adjacency(const uint64_t* uniq, uint64_t n_keys, uint32_t shift, const Adj& a, uint64_t* rank_keys, unsigned long long* counters,
                           hipStream_t s) {
    hipLaunchKernelGGL(offsets_kernel, dim3(blocks_for((uint64_t)a.V + 1)), dim3(kBlock), 0, s, uniq, shift, a, counters);
    const uint64_t n = n_keys > a.V ? n_keys : a.V;
    if (n) hipLaunchKernelGGL(neighbours_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, uniq, n_keys, shift, a, rank_keys, counters);
    return hipGetLastError();
}

hipError_t classify(const uint64_t* sorted_rank_keys, const Adj& a, uint64_t* cnt_c, uint64_t* cnt_e, unsigned long long* counters, hipStream_t s) {
    if (a.V) hipLaunchKernelGGL(rank_kernel, dim3(blocks_for(a.V)), dim3(kBlock), 0, s, sorted_rank_keys, a);
    hipLaunchKernelGGL(classify_kernel, dim3(blocks_for((uint64_t)a.V + 1)), dim3(kBlock), 0, s, a, cnt_c, cnt_e, counters);
    return hipGetLastError();
}

hipError_t count_pass(const Adj& a, uint64_t* cnt_c, uint64_t* cnt_e, uint64_t* scratch, uint32_t n_waves, uint32_t dmax, uint64_t budget,
                      unsigned long long* counters, hipStream_t s) {
    hipLaunchKernelGGL(bk_kernel<false>, dim3(n_waves / (kBlock / 64)), dim3(kBlock), 0, s, a, cnt_c, cnt_e, scratch, dmax, budget, counters,
                       (unsigned long long*)nullptr, (uint32_t*)nullptr);
    return hipGetLastError();
}

hipError_t write_pass(const Adj& a, const uint64_t* cnt_c, const uint64_t* cnt_e, uint64_t* scratch, uint32_t n_waves, uint32_t dmax,
                      unsigned long long* counters, unsigned long long* clique_off, uint32_t* clique_nodes, hipStream_t s) {
    hipLaunchKernelGGL(write_trivial_kernel, dim3(blocks_for((uint64_t)a.V + 1)), dim3(kBlock), 0, s, a, cnt_c, cnt_e, clique_off, clique_nodes);
    if (dmax)
        hipLaunchKernelGGL(bk_kernel<true>, dim3(n_waves / (kBlock / 64)), dim3(kBlock), 0, s, a, const_cast<uint64_t*>(cnt_c), const_cast<uint64_t*>(cnt_e),
                           scratch, dmax, ~0ull, counters, clique_off, clique_nodes);
    return hipGetLastError();
}

}  // namespace cliques
}  // namespace hc
