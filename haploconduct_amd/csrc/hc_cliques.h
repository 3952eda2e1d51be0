// hc_cliques.h — what the kernels (hc_cliques_kernels.hip), the glue (hc_api_cliques.cpp) and the host mirror (host/Cliques.cpp) of
// hc_graph_cliques (include/hcedge.h) share: the counters, the packed pair keys, the per-wave scratch layout, the launch interface
// and the host's per-root routine.  The order rule itself is host/CliqueRule.h.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <vector>

#include "../../include/hcedge.h"
#include "host/CliqueRule.h"

namespace hc {
namespace cliques {

// A pair (i, j) as one key: i << shift | j with 2^shift >= V; an out-record that gives no pair is kSkip(shift) = 1 << 2 * shift, which
// sorts behind every pair (V < 2^31: at most 63 bits).
inline uint32_t key_shift(uint64_t V) {
    uint32_t b = 1;
    while ((1ull << b) < V) b++;
    return b;
}

// counters[]: the first failed assert (hc_graph_text.h: bad_key, kNoKey), then tallies
enum { kKey = 0, kUnique = 1, kMaxDeg = 2, kHostRoots = 3, kSingletons = 4, kTicket = 5, kTotal = 6, kOver = 7, kMaxClique = 8, kCounters = 16 };
// per root (indexed by rank): 0 trivial (counted by the classify pass), 1 a wave's, 2 the host's
enum { kRootTrivial = 0, kRootDevice = 1, kRootHost = 2 };

// A wave's scratch for roots of degree <= dmax, in 64-bit words: the matrix, dmax + 1 stack levels of P, X and the candidates, R, and
// the vertex each level took.
HC_CLQ_HD inline uint64_t slice_words(uint32_t dmax) {
    const uint64_t W = words_of(dmax);
    return (uint64_t)dmax * W + ((uint64_t)dmax + 1) * 3 * W + W + ((uint64_t)dmax + 2) / 2 + 1;
}

// The simple adjacency on the host: off (V + 1), nbr ascending per vertex, rank.
struct HostAdj {
    const uint64_t* off;
    const uint32_t* nbr;
    const uint32_t* rank;
};
// One root's cliques in the rule's order, appended: a size per clique, the vertices ascending.  *entries grows by what was appended;
// false: it passed `budget` and the root was abandoned.
bool host_root(const HostAdj& a, uint32_t v, uint64_t budget, std::vector<uint32_t>& sizes, std::vector<uint32_t>& nodes, uint64_t* entries,
               uint32_t* max_clique);

#if defined(__HIPCC__)
struct Graph {  // the context's graph
    const hc_edge_rec* E;
    const unsigned long long* out_off;
    const uint8_t* incl;
    uint32_t V, n_edges;
};
struct Adj {  // the simple adjacency on the device
    unsigned long long* off;  // V + 1
    uint32_t* nbr;            // off[V] of them (room for 2 * n_edges)
    uint32_t* rank;           // V
    uint32_t* order;          // V: the vertex of each rank
    uint8_t* kind;            // V, by rank: kRoot*
    uint32_t V, cap;
};
// keys[2 * n_edges] <- the records' pairs, both ways, or kSkip; the assert scan goes into counters[kKey]
hipError_t emit_pairs(const Graph& g, uint32_t shift, uint64_t* keys, unsigned long long* counters, hipStream_t s);
// off / nbr from the sorted distinct keys (counters[kUnique] of them, kSkip last if present); rank_keys[V] <- rank_key(degree, v)
hipError_t build_adjacency(const uint64_t* uniq, uint64_t n_keys, uint32_t shift, const Adj& a, uint64_t* rank_keys, unsigned long long* counters,
                           hipStream_t s);
// rank / order from the sorted rank keys; then kind[] and the trivial roots' counts (cnt_c / cnt_e by rank, V + 1 each, the last 0)
hipError_t classify(const uint64_t* sorted_rank_keys, const Adj& a, uint64_t* cnt_c, uint64_t* cnt_e, unsigned long long* counters, hipStream_t s);
// The waves' roots.  count: cnt_c / cnt_e receive each root's cliques and entries.  write: they hold the exclusive sums, and every
// clique goes to its place in clique_off / clique_nodes; the trivial roots' cliques and clique_off[n_cliques] too.
hipError_t count_pass(const Adj& a, uint64_t* cnt_c, uint64_t* cnt_e, uint64_t* scratch, uint32_t n_waves, uint32_t dmax, uint64_t budget,
                      unsigned long long* counters, hipStream_t s);
hipError_t write_pass(const Adj& a, const uint64_t* cnt_c, const uint64_t* cnt_e, uint64_t* scratch, uint32_t n_waves, uint32_t dmax,
                      unsigned long long* counters, unsigned long long* clique_off, uint32_t* clique_nodes, hipStream_t s);
#endif

}  // namespace cliques
}  // namespace hc
