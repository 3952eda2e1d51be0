// Cycles.h — the host's share of OverlapGraph::cycleRemovalHeuristic (src/GraphAlgos.cpp:352-541), used by the mirror
// (hc_host_graph_remove_cycles) and by hc_graph_remove_cycles: the iterative walk over a target column, the target columns of the 20
// tries from flat records (plain sorts; the device builds its own), the permutation table the device gathers through, and sortEdges'
// treatment of one flat out-list (hc_graph_sort_edges' tied lists).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../../include/hcedge.h"

namespace hc {
namespace cycles {

constexpr uint32_t kTries = HC_CYCLES_TRIES;  // `while (count < 20 && opt_backedge_vec.size() > 0)`, :517
constexpr uint32_t kFirstShuffle = 5;         // tries 5 .. 20 shuffle, :467-474

// findCycles' walk (:487-506 with dfs_helper, :352-485) over one try's neighbour order: roots in visiting order, off (V + 1) and col
// the CSR of the reordered targets.  An explicit stack of (vertex, next position) stands for the recursion, which would overflow on a
// path of 10^6 vertices.  pairs: the back edges u << 32 | v, sorted and unique (the reference's std::set in its order).
void walk(const uint32_t* roots, uint64_t n_roots, const uint64_t* off, const uint32_t* col, uint32_t V, std::vector<uint64_t>& pairs);

// sortVerticesByIndegree (:150-176) from the in-list offsets
void roots_by_indegree(const uint64_t* in_off, uint32_t V, std::vector<uint32_t>& roots);

// The targets of every out-list in the order try t (1 .. 20) visits them (:377-474), from flat records in list order.
void target_column(const hc_edge_rec* edges, const uint64_t* out_off, uint32_t V, uint32_t t, std::vector<uint32_t>& col);

// 16 rows of len entries: row t - 5 is the permutation std::srand(t); std::random_shuffle applies to len elements
void perm_table(uint32_t len, uint32_t* table);

// Tries first .. last over one CSR of target columns (cols[t - first]: the column of try t) on n_threads threads, one try per task:
// sets[t - first] = walk(...)
void walk_tries(const uint32_t* roots, uint64_t n_roots, const uint64_t* off, const uint32_t* const* cols, uint32_t V, uint32_t first, uint32_t last,
                unsigned n_threads, std::vector<uint64_t>* sets);

// OverlapGraph::sortEdges' treatment of one out-list (src/OverlapGraph.cpp:724-749) on n flat records in their incoming order, seq
// (may be null) following them: host_model.cpp's sort_out_list with the same key, comparator and std::sort
void sort_out_list(hc_edge_rec* list, uint32_t* seq, size_t n, const uint32_t* len_by_read);

}  // namespace cycles
}  // namespace hc
