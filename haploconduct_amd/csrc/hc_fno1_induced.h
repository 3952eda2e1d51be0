// hc_fno1_induced.h — findInclusionOverlaps' arithmetic (reference src/FindNextOverlaps.cpp:816-887) in one place: the host's
// collect_induced (host/FindNextOverlaps.cpp) and the device's pair kernels (hc_fno1_resident_kernels.hip) both call it.  Plain C++ that
// also compiles as device code; R is any record with v1, v2, pos1, ori1, ori2 (hc_fno_edge, hc_edge_rec).
#ifndef HC_FNO1_INDUCED_H_
#define HC_FNO1_INDUCED_H_
#include <cmath>
#include <cstdint>

#include "../../include/hcfno.h"
#include "hc_fno_items.h"

namespace hc {
namespace fno1i {

enum Verdict : int {
    kSkip = 0,       // the pair induces no edge u -> v (:841-843, :862-865), or a paired read is involved (:867-869)
    kCandidate = 1,  // *ne is the induced edge; the caller asks checkEdge(ne->v1, ne->v2, true) == -1
    // the reference stops:
    kStopRelation = 2,   // assert(edge1.get_vertex(2) == edge2.get_vertex(2)), :863
    kStopVertex = 3,     // a vertex the graph does not have
    kStopZeroLen = 4,    // a read of length 0: the division of :871
    kStopThreshold = 5,  // Edge's constructor (src/Edge.h:46) on program_settings.edge_threshold
    kStopLen = 6         // Edge::set_len: len > 0
};

// pairs (i, j), i < j, of a group of l records
HC_FNO_HD inline uint64_t pairs_of(uint64_t l) { return l ? l * (l - 1) / 2 : 0; }

// Pair t of a group of l records in (i, j) order, i < j: i is the largest row with first(i) <= t, first(i) = i (2 l - i - 1) / 2.  A
// floating root gives a first guess only; the row is verified and adjusted in integer arithmetic.
HC_FNO_HD inline void pair_of(uint64_t t, uint64_t l, uint32_t* i_out, uint32_t* j_out) {
    const double b = 2.0 * (double)l - 1.0;
    const double disc = b * b - 8.0 * (double)t;
    const double root = disc > 0.0 ? sqrt(disc) : 0.0;
    const double guess = (b - root) * 0.5;
    uint64_t i = guess > 0.0 ? (uint64_t)guess : 0;
    if (i > l - 2) i = l - 2;
    while (i > 0 && i * (2 * l - i - 1) / 2 > t) i--;
    while (i + 1 <= l - 2 && (i + 1) * (2 * l - i - 2) / 2 <= t) i++;
    *i_out = (uint32_t)i;
    *j_out = (uint32_t)(t - i * (2 * l - i - 1) / 2 + i + 1);
}

// :841-875 for the records e1 = group[i], e2 = group[j].
template <typename R>
HC_FNO_HD inline int induced_edge(const R& e1, const R& e2, const hc_fno_read* nodes, uint64_t n_nodes, double edge_threshold, hc_fno_edge* ne) {
    const R *head, *tail;  // head->v1 = u, tail->v2 = v: u -> w and w -> v are both inclusions, try u -> v
    if (e1.v1 == e2.v1) return kSkip;
    if (e1.v1 == e2.v2) {
        head = &e2;
        tail = &e1;
    } else if (e1.v2 == e2.v1) {
        head = &e1;
        tail = &e2;
    } else {
        return e1.v2 == e2.v2 ? kSkip : kStopRelation;
    }
    if (head->v1 >= n_nodes || tail->v2 >= n_nodes) return kStopVertex;
    const hc_fno_read &r1 = nodes[head->v1], &r2 = nodes[tail->v2];
    if (r1.paired || r2.paired) return kSkip;
    // std::min(read1->get_len() - pos1, read2->get_len()) with get_len() unsigned: the difference wraps where pos1 exceeds the length
    const unsigned L1 = r1.len1, L2 = r2.len1;
    const unsigned d = L1 - (unsigned)head->pos1;
    const int len = (int)(d < L2 ? d : L2);
    const unsigned shorter = L1 < L2 ? L1 : L2;
    if (shorter == 0) return kStopZeroLen;
    const int perc = (int)((100u * (unsigned)len) / shorter);
    if (!(edge_threshold == 0 || edge_threshold == -1 || edge_threshold > 0)) return kStopThreshold;
    if (!(len > 0)) return kStopLen;
    hc_fno_edge o;
    o.v1 = head->v1;
    o.v2 = tail->v2;
    o.score = edge_threshold;
    o.pos1 = head->pos1;
    o.pos2 = 0;
    o.len1 = len;
    o.len2 = 0;
    o.perc = perc;
    o.ord = '-';
    o.ori1 = head->ori1;
    o.ori2 = tail->ori2;
    o.pad = 0;
    *ne = o;
    return kCandidate;
}

}  // namespace fno1i
}  // namespace hc
#endif
