// Labelling.h — the host's share of OverlapGraph::vertexLabellingHeuristic (src/GraphAlgos.cpp:178-349), used by the mirror
// (hc_host_graph_label_vertices) and by hc_graph_label_vertices for the components that hold an odd cycle: Edge::switch_edge_orientation
// on a flat record, the reference's shuffle restated with a state of its own, and the BFS tries over a compact subgraph.
#pragma once
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "../../../include/hcedge.h"

#if defined(__HIPCC__)
#define HC_LABEL_HD __host__ __device__
#else
#define HC_LABEL_HD
#endif

namespace hc {
namespace label {

constexpr uint32_t kTries = 100;  // `while (count < 100 && delete_count > 0)`, :204

// Edge::switch_edge_orientation (src/Edge.h:90-121) on a flat record; read1 / read2 travel with the vertices.  true: the record changed
// direction and belongs to the other vertex's list.
HC_LABEL_HD inline bool switch_edge_orientation(hc_edge_rec& e) {
    int32_t t = e.pos1;
    e.pos1 = e.pos3, e.pos3 = t;
    t = e.pos2, e.pos2 = e.pos4, e.pos4 = t;
    e.ori1 = !e.ori1;
    e.ori2 = !e.ori2;
    if (e.pos1 < 0 || (e.pos1 == 0 && e.v1 > e.v2)) {
        const uint32_t r = e.read1;
        e.read1 = e.read2, e.read2 = r;
        const uint64_t v = e.v1;
        e.v1 = e.v2, e.v2 = v;
        const uint8_t o = e.ori1;
        e.ori1 = e.ori2, e.ori2 = o;
        e.pos1 = -e.pos1;
        if (e.pos2 < 0) {
            e.ord = '1';
            e.pos2 = -e.pos2;
        } else if (e.ord != '-') {
            e.ord = '2';
        }
        return true;
    }
    if (e.pos2 < 0) {
        e.pos2 = -e.pos2;
        e.ord = '2';
    } else if (e.ord != '-') {
        e.ord = '1';
    }
    return false;
}

// glibc's srand / rand (the additive-feedback generator, TYPE_3: degree 31, separation 3, 310 values discarded after seeding) with a
// state of its own: the library never touches its caller's generator.
class GlibcRand {
public:
    explicit GlibcRand(unsigned int seed) { srand(seed); }
    void srand(unsigned int seed);
    int rand() {
        const uint32_t x = r_[front_] += r_[back_];
        front_ = (front_ + 1) % 31;
        back_ = (back_ + 1) % 31;
        return (int)(x >> 1);
    }

private:
    uint32_t r_[31];
    uint32_t front_ = 3, back_ = 0;
};

// The permutation std::srand(seed); std::random_shuffle(first, first + n) applies (libstdc++: for i = 1 .. n - 1, j = rand() % (i + 1),
// swap if i != j): element i of the result is element perm[i] of the input.  A function of (seed, n) alone.
void shuffle_permutation(unsigned int seed, uint32_t n, std::vector<uint32_t>& perm);

// The permutations of one seed, by length.
class ShuffleCache {
public:
    explicit ShuffleCache(unsigned int seed) : seed_(seed) {}
    const std::vector<uint32_t>& get(uint32_t n) {
        auto it = by_len_.find(n);
        if (it == by_len_.end()) {
            it = by_len_.emplace(n, std::vector<uint32_t>()).first;
            shuffle_permutation(seed_, n, it->second);
        }
        return it->second;
    }

private:
    unsigned int seed_;
    std::unordered_map<uint32_t, std::vector<uint32_t>> by_len_;
};

// The vertices of the components that hold an odd cycle, renumbered 0 .. n - 1 in ascending vertex order, with their lists in list
// order: adj_in (in_nb), the targets of adj_out (out_nb) and the records' class, ori1 == ori2 (out_same).
struct Subgraph {
    uint32_t n;
    const uint64_t *in_off, *out_off;  // n + 1 each
    const uint32_t *in_nb, *out_nb;
    const uint8_t* out_same;
};
// labelVertices' BFS (:252-290) for seeds 1 .. n_tries on n_threads threads: bit t - 1 of bits[2 v] (tries 1 - 64) or bits[2 v + 1]
// (65 - 100) is orientations[v] of try t.  bits: 2 n words, zeroed here.
void label_tries(const Subgraph& S, uint32_t n_tries, unsigned n_threads, uint64_t* bits);

}  // namespace label
}  // namespace hc
