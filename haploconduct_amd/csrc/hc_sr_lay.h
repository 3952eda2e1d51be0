// hc_sr_lay.h — what the pair kernel (hc_sr_edge_kernels.hip) and the clique kernels (hc_sr_clique_kernels.hip) share of
// sort_vertices (reference src/SRBuilder.cpp:33-285), so that the two cannot drift: getEdgeInfo's scan of one list, the base's
// member, the per-node part of the loop (:92-240) and calcSubreadInfo's placement (:548-568).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr.h"

namespace hc {
namespace srlay {

constexpr uint32_t kNone = 0xffffffffu;

// The first k in [a, b) with E[k].v2 == target, or kNone; every lane of the wave calls it (a == b: nothing to find).  A lane walks a
// list of fewer than 64 records, the wave walks a longer one 64 records at a time and stops at the first chunk with a hit.
__device__ inline uint32_t find_first(const hc_edge_rec* __restrict__ E, uint32_t a, uint32_t b, uint32_t target, uint32_t lane) {
    uint32_t hit = kNone;
    const bool is_long = b - a >= 64;
    if (!is_long)
        for (uint32_t k = a; k < b; k++)
            if (E[k].v2 == target) {
                hit = k;
                break;
            }
    unsigned long long longs = __ballot(is_long);
    while (longs) {
        const int j = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const uint32_t aj = __shfl(a, j), bj = __shfl(b, j), tj = __shfl(target, j);
        uint32_t found = kNone;
        for (uint32_t base = aj; base < bj; base += 64) {  // (wave-uniform: aj, bj and the ballot are)
            const uint32_t k = base + lane;
            const unsigned long long m = __ballot(k < bj && E[k].v2 == tj);
            if (m) {
                found = base + (uint32_t)(__ffsll((long long)m) - 1);
                break;
            }
        }
        if ((int)lane == j) hit = found;
    }
    return hit;
}

struct FoundEdge {
    uint32_t read1, read2;
    int32_t pos1, pos2;
    uint8_t ord;
};

// the base's member of a layout of `type` (:47-76); its position is 0
__device__ inline hc_sr_member base_member(char type, uint32_t base_ID, bool base_fwd) {
    hc_sr_member m;
    m.read = base_ID;
    m.pos = 0;
    m.pad[0] = m.pad[1] = 0;
    m.rev = base_fwd ? 0 : 1;
    m.seq = type == 's' ? 0 : ((type == 'l') == base_fwd ? 1 : 2);
    return m;
}

// What one pass of the loop (:87-242) inserts for `node`: n = 1 entry, or 2 (mate 1, then mate 2) for a paired read in an 's' layout;
// positions before the shift; len1 / len2 of :225-238.
struct NodeLay {
    uint32_t n;
    int64_t pos[2];
    uint32_t len[2];
    hc_sr_member m[2];
    int64_t len1, len2;
};

// :101-238 for the record found.  Returns HC_SR_EDGE_* in the reference's order of checks.
__device__ inline uint32_t lay_node(const StoreView& st, char type, uint32_t base_ID, int64_t base_len, bool node_fwd, const FoundEdge& e, NodeLay& o) {
    const bool base_is_1 = e.read1 == base_ID, base_is_2 = e.read2 == base_ID;
    if (!base_is_1 && !base_is_2) return HC_SR_EDGE_READ_MISMATCH;  // :108
    const uint32_t current_id = base_is_1 ? e.read2 : e.read1;      // :104-110
    if (current_id >= st.n_reads) return HC_SR_EDGE_BAD_VERTEX;
    const ReadDesc cd = st.reads[current_id];
    const bool cur_paired = (cd.flags & kReadPaired) != 0;
    char current_type = type;
    if (type == 's') current_type = cur_paired ? 'p' : 's';  // :114-122
    else if (!cur_paired) return HC_SR_EDGE_READ_MISMATCH;    // src/Read.h:145-149
    const int64_t p1 = base_is_1 ? (int64_t)e.pos1 : -(int64_t)e.pos1;  // :142-147, :159-164
    int64_t new_pos = p1;
    const int64_t new_pos1 = p1;
    hc_sr_member m;
    m.read = current_id;
    m.pos = 0;
    m.pad[0] = m.pad[1] = 0;
    m.rev = node_fwd ? 0 : 1;
    if (current_type == 's') m.seq = 0;
    else m.seq = node_fwd ? 1 : 2;  // :151-158
    uint32_t n = 0;
    if (current_type == 'p') {
        o.pos[n] = new_pos1;
        o.len[n] = m.seq == 2 ? cd.len2 : cd.len1;
        o.m[n] = m;
        n++;
    }
    if (current_type == 'r' || current_type == 'p') {  // :171-188
        m.seq = node_fwd ? 2 : 1;
        if (current_type == 'p' || (base_is_1 && e.ord == '1') || (base_is_2 && e.ord == '2')) new_pos = e.pos2;
        else new_pos = -(int64_t)e.pos2;
    }
    o.pos[n] = new_pos;
    o.len[n] = m.seq == 2 ? cd.len2 : cd.len1;
    o.m[n] = m;
    n++;
    o.n = n;
    if (current_type == 'p') {  // :225-238
        if (new_pos < 0) return HC_SR_EDGE_PAIRED_NEG_POS;  // :227
        o.len1 = -new_pos1;
        o.len2 = max((int64_t)o.len[1] + new_pos - base_len, (int64_t)o.len[0] + new_pos1 - base_len);
    } else {
        o.len1 = -new_pos;
        o.len2 = (int64_t)o.len[0] + new_pos - base_len;
    }
    return HC_SR_EDGE_OK;
}

// :548-555 / :561-568 / :583-590: (index, startpos) of an entry at `pos` under trim position `trim`
__device__ inline void sub_place(int32_t trim, int32_t pos, int32_t& index, int32_t& startpos) {
    if (trim > pos) {
        startpos = trim - pos;
        index = 0;
    } else {
        startpos = 0;
        index = pos - trim;
    }
}

}  // namespace srlay
}  // namespace hc
