// hc_trans.h — launch interface of hc_trans_kernels.hip (OverlapGraph::removeInclusions + removeTransitiveEdges on the
// device).  The one host step of the device route, std::sort's order of an out-list by target, is host/TargetOrder.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"
#include "host/TargetOrder.h"

namespace hc {

namespace trans {

// A device graph in CSR form: adj_out records back to back in vertex order (E of them, list order) with seq (one per
// record) and out_off (V + 1); adj_in as in_nodes with in_off (V + 1).
struct Graph {
    hc_edge_rec* edges;
    uint32_t* seq;
    unsigned long long* out_off;
    uint32_t* in_nodes;
    unsigned long long* in_off;
    uint32_t V, E;
};

// Scratch of one call for E edges and V vertices.
size_t temp_bytes(uint64_t E, uint64_t V);

// hc_graph_load's checks on the device: every record lies in the list of its vertex1, every id < V, adj_in holds the
// same (source, target) pairs as adj_out.  The offsets must already span [0, E] without decreasing (the caller checks).
// Writes g.seq = 0, 1, ...
hipError_t check_graph(const Graph& g, bool* consistent, void* temp, size_t temp_bytes, hipStream_t s);
// removeTransitiveEdges from `in` into `out` (distinct buffers, room for in.E edges; out.E is set).  Synchronous on s:
// the host takes part twice (the lists std::sort orders differently from a stable sort, and the branch choice).
hipError_t remove_transitive(const Graph& in, Graph& out, uint32_t remove_trans, uint32_t branch_reduction, hc_clean_counts* counts, void* temp,
                             size_t temp_bytes, hipStream_t s);
// removeInclusions from `in` into `out`; the groups: group_vertex (room for V), group_off (V + 1), group_edges (2 E).
hipError_t remove_inclusions(const Graph& in, const uint8_t* inclusions, Graph& out, uint32_t* group_vertex, unsigned long long* group_off,
                             hc_edge_rec* group_edges, uint64_t* n_groups, uint64_t* n_group_edges, hc_clean_counts* counts, void* temp,
                             size_t temp_bytes, hipStream_t s);
// removeTips / removeBranches in two steps, because the caller sizes branching_edges between them.  find_* leaves in the
// scratch which records and in-entries stay and the list of removed records in removal order, and fills the counts but
// edges_after; commit_removed (same graph, same scratch, nothing in between) appends the n_removed records to `removed`
// and writes the cleaned graph into `out` (target_ordered: find_branches' lists, in sortAdjOut's order).  in.E > 0.
// find_tips: tip = the per-read flags (n_flags >= n_reads bytes, set where a read becomes a tip); *reads_in_range false: a record
// names a read >= n_reads and nothing else was done.
hipError_t find_tips(const Graph& in, uint32_t max_tip_len, const hc_read_geom* reads, uint64_t n_reads, uint8_t* tip, uint64_t n_flags, hc_tip_counts* counts,
                     bool* reads_in_range, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t find_branches(const Graph& in, hc_branch_counts* counts, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t commit_removed(const Graph& in, Graph& out, bool target_ordered, hc_edge_rec* removed, uint64_t n_removed, void* temp, size_t temp_bytes,
                          hipStream_t s);
// OverlapGraph::removeEdge for n listed records (hc_br_reduce): the records rec[k] of `in` (distinct) leave with the adj_in entries in_pos[k]
// (distinct); removed[k] = record rec[k], and the rest goes to `out` with both lists in the order they had (the compaction of
// commit_removed).  in.E > 0.
hipError_t remove_records(const Graph& in, Graph& out, const uint32_t* rec, const uint32_t* in_pos, uint32_t n, hc_edge_rec* removed, void* temp,
                          size_t temp_bytes, hipStream_t s);
// sortAdjOut alone (hc_br_evidence): the records and seq of `in` in sortAdjOut's order — the target-order step of find_branches, its host
// step for lists that repeat a target included — into out.edges / out.seq (room for in.E).  The order changes inside lists only: the
// offsets and adj_in are not touched.  in.E > 0.
hipError_t sort_adj_out(const Graph& in, Graph& out, uint64_t* n_tied_lists, void* temp, size_t temp_bytes, hipStream_t s);

}  // namespace trans
}  // namespace hc
