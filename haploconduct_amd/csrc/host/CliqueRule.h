// CliqueRule.h — the order rule of hc_graph_cliques / hc_host_graph_cliques (include/hcedge.h, "maximal cliques of the device graph")
// in one place for the host (host/Cliques.cpp) and the device (hc_cliques_kernels.hip): the rank key, which neighbours start in P, a
// row of the root's bit matrix, the pivot's choice, the candidates and the emit test.  The traversals around them differ (a wave works
// over words and members, the host is one loop); what they decide with is here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HC_CLQ_HD __host__ __device__
#else
#define HC_CLQ_HD
#endif

namespace hc {
namespace cliques {

// rank(v) = the position of v in ascending (degree, id)
HC_CLQ_HD inline uint64_t rank_key(uint32_t degree, uint32_t v) { return (uint64_t)degree << 32 | v; }
// A root's universe: its d neighbours in ascending id, as local indices 0 .. d - 1; a set over them has words_of(d) words.
HC_CLQ_HD inline uint32_t words_of(uint32_t d) { return (d + 63u) >> 6; }
// Neighbour u of root v starts in P iff it ranks above v, in X otherwise.
HC_CLQ_HD inline bool starts_in_P(uint32_t rank_u, uint32_t rank_v) { return rank_u > rank_v; }

// Row a of the matrix: the local indices of N(u) & N(v), u = Nv[a].  Both lists ascend and hold no repeats; u is not in N(u), so the
// diagonal stays clear.  A walk over both lists, or, where N(u) is much the longer one, a search in it per member of N(v).
HC_CLQ_HD inline void matrix_row(const uint32_t* Nu, uint32_t du, const uint32_t* Nv, uint32_t d, uint64_t* row) {
    const uint32_t W = words_of(d);
    for (uint32_t w = 0; w < W; w++) row[w] = 0;
    if (du > 16u * d) {
        for (uint32_t b = 0; b < d; b++) {
            const uint32_t t = Nv[b];
            uint32_t lo = 0, hi = du;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (Nu[mid] < t) lo = mid + 1;
                else hi = mid;
            }
            if (lo < du && Nu[lo] == t) row[b >> 6] |= 1ull << (b & 63u);
        }
        return;
    }
    uint32_t i = 0, b = 0;
    while (i < du && b < d) {
        const uint32_t x = Nu[i], y = Nv[b];
        if (x == y) row[b >> 6] |= 1ull << (b & 63u);
        i += x <= y;
        b += y <= x;
    }
}

// The pivot: the member of P | X with the most neighbours in P, ties to the smallest local index = the largest key.  0 is no key.
HC_CLQ_HD inline uint64_t pivot_key(uint32_t neighbours_in_P, uint32_t idx) { return (uint64_t)neighbours_in_P << 32 | (0xffffffffu - idx); }
HC_CLQ_HD inline uint32_t pivot_of(uint64_t key) { return 0xffffffffu - (uint32_t)key; }
// The candidates of a node, word by word: P \ N(pivot), taken in ascending local index, each moved from P to X after its sub-tree.
HC_CLQ_HD inline uint64_t candidates(uint64_t P_word, uint64_t pivot_row_word) { return P_word & ~pivot_row_word; }
// A node with P = {} reports R iff X = {} too.
HC_CLQ_HD inline bool emits(bool any_P, bool any_X) { return !any_P && !any_X; }

}  // namespace cliques
}  // namespace hc
