// hc_fno1_resident.h — what the kernels (hc_fno1_resident_kernels.hip) and the glue (hc_api_fno1_resident.cpp, hc_api_fno.cpp) of
// hc_fno1_from_graph (include/hcsr.h) share: the views of the context's graph, the counters and the launch interface.
//
// The walk's edge list is [adj_out][branching_edges][stored non-edges that pass :694][inclusion-induced edges] (reference
// src/FindNextOverlaps.cpp:612-630, :635-813, :816-887).  Segments 1 and 2 are conversions of the graph's 80-byte records; 3 and 4 are
// decided by OverlapGraph::checkEdge (src/OverlapGraph.cpp:233-259) against segment 1 and the graph's out_off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"
#include "../../include/hcfno.h"
#include "hc_fno_items.h"

namespace hc {
namespace fno1r {

constexpr uint64_t kMaxCount = 0x7FFFFFF0ull;  // 2^31 - 16: what the walk's 32-bit indices hold
constexpr uint32_t kLaneList = 64;             // a lane scans out-lists shorter than this; a wave takes the longer ones, 64 records at a time

// counts[]: what the ordered selections count (written once each, by select_flagged)
enum { kLongNon = 0, kKeptNon = 1, kLongInd = 2, kKeptInd = 3, kCounts = 8 };

struct Adj {  // adj_out as the walk sees it: the converted records and the graph's offsets
    const hc_fno_edge* edges;
    const unsigned long long* out_off;  // n_nodes + 1
    const hc_fno_read* nodes;
    uint64_t n_nodes;
};
struct Groups {  // OverlapGraph::inclusion_edges, group by group, and the pairs (i < j) in front of every group
    const hc_edge_rec* edges;
    const uint64_t* off;       // n_groups + 1
    const uint64_t* pair_off;  // n_groups + 1: the exclusive sum of l (l - 1) / 2
    uint64_t n_groups;
    double edge_threshold;
};

// out[k] = in[k] field by field (v1, v2, score, pos1, pos2, len1, len2, perc, ord, ori1, ori2); both arrays 16-byte aligned
hipError_t convert(const hc_edge_rec* in, uint64_t n, hc_fno_edge* out, hipStream_t s);
// cnt[g] = l (l - 1) / 2 for g < n_groups, cnt[n_groups] = 0
hipError_t group_pairs(const uint64_t* off, uint64_t n_groups, uint64_t* cnt, hipStream_t s);
// Stored non-edge i: keep[i] = 1 unless checkEdge(v1, v2, true) > 0; is_long[i] = 1 where a wave has to decide (keep[i] is then 0 so far).
// A record that is no stored non-edge, or one the reference stops at, sets status[4] (hc_fno_device.h: kFnoStatus*).
hipError_t nonedge_lanes(const hc_fno_edge* non, uint64_t n, const Adj& a, uint8_t* keep, uint8_t* is_long, unsigned long long* status, hipStream_t s);
hipError_t nonedge_waves(const hc_fno_edge* non, const uint32_t* long_idx, const unsigned long long* n_long, const Adj& a, uint8_t* keep, uint32_t n_cu,
                         hipStream_t s);
// Pair t of the groups: keep[t] = 1 where the pair induces an edge and checkEdge(node1, node2, true) == -1
hipError_t induced_lanes(const Groups& g, uint64_t n_pairs, const Adj& a, uint8_t* keep, uint8_t* is_long, unsigned long long* status, hipStream_t s);
hipError_t induced_waves(const Groups& g, const uint32_t* long_idx, const unsigned long long* n_long, const Adj& a, uint8_t* keep, uint32_t n_cu,
                         hipStream_t s);
// out[k] = the induced edge of pair idx[k]
hipError_t induced_build(const Groups& g, const uint32_t* idx, uint64_t n, const Adj& a, hc_fno_edge* out, hipStream_t s);
// The super-read tables: every clique holds a vertex (get_sorted_clique asserts it); entry e of the subread maps -> the key
// super-read << 32 | node and the value e; then out[p] = subreads[val_sorted[p]]
hipError_t cliques_check(const uint64_t* clique_off, uint64_t n_srs, unsigned long long* status, hipStream_t s);
hipError_t subread_keys(const uint64_t* subread_off, const hc_fno_subread* subreads, uint64_t n_srs, uint64_t total, uint64_t* key, uint32_t* val,
                        unsigned long long* status, hipStream_t s);
hipError_t subread_gather(const hc_fno_subread* subreads, const uint32_t* val_sorted, uint64_t total, hc_fno_subread* out, hipStream_t s);
// The unique lines as records: head[i] = len[i] != 0 (head[n] = 0); after its exclusive sum, the record at sorted place i goes to
// lines[rank[i]] with the columns of the text
hipError_t line_heads(const uint64_t* len, uint64_t n, uint32_t* head, hipStream_t s);
hipError_t line_records(const FnoRec* rec, const uint32_t* perm, const uint64_t* len, const uint32_t* rank, uint64_t n, hc_line_rec* lines,
                        uint64_t n_lines, hipStream_t s);

}  // namespace fno1r
}  // namespace hc
