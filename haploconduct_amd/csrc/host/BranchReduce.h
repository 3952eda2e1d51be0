// BranchReduce.h — what hc_br_reduce (hc_api_br.cpp) and its host mirror hc_host_br_reduce (host/BranchReduce.cpp) share: the serial,
// order-dependent part of the second half of BranchReduction::readBasedBranchReduction (reference src/BranchReduction.cpp:82-227,
// :745-1272) — the component walk, the threshold look-up, the diploid rule and the --careful chain — ONE source for both.  The maps the
// result's order depends on are real std::unordered_map objects keyed by the reference's node_id_t (unsigned long) and
// safe_edge_count_t (unsigned long long), filled with the reference's inserts in the reference's order, so they iterate as the
// reference's do under the same standard library (include/hcsr.h says what that pins).  Plain C++: builds without HIP.
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/hcsr.h"

namespace hc {
int set_last_error(int status, const std::string& what);  // (hc_scratch.h)

namespace brr {

typedef unsigned long node_id_t;                          // src/Types.h:94
typedef unsigned long long safe_edge_count_t;             // src/Types.h:96
typedef std::pair<node_id_t, node_id_t> node_pair_t;      // src/Types.h:97

// getEdgeInfo's record for a final_branch neighbour (one per branch_nb entry): Read::get_len() of its read1 and read2, and get_len(0)
struct Triple {
    int32_t len1, len2, olen;
};

struct Components {
    std::vector<hc_br_component> comps;     // branching_components: dist, edge_first, edge_count; the rest 0 until run_chain
    std::vector<node_pair_t> edges;         // their edges, component by component
    std::vector<uint8_t> typical;           // per component: the typical double branch of :1045
    std::vector<node_pair_t> to_remove;     // edges_to_remove, in push order until finish_removals sorts it
    uint64_t n_false_dropped = 0;
};

// findBranchingComponents with extendComponentOut / extendComponentIn (:745-1007).  tri: per branch_nb entry.  nullptr: fine; else what is
// wrong with the tables (a neighbour or node >= V, nb_first + nb_count beyond n_nb).
const char* find_components(const hc_br_branch* branches, uint64_t n_branches, const uint32_t* branch_nb, uint64_t n_nb, const Triple* tri, uint64_t V,
                            Components& out);

// host_finished bits every component has before any evidence is looked at: HC_BR_RED_HOST_SHARED_EDGE (one sort of all component edges)
// and, under diploid, HC_BR_RED_HOST_DIPLOID
void mark_host_finished(Components& c, bool diploid);

// evidence_threshold_map.find(dist) for every component (:182): found and min_evidence (-1 where not found)
void look_up_thresholds(const hc_br_reduce_settings* st, const Components& c, std::vector<int32_t>& min_evidence, std::vector<uint8_t>& found);

// The rule of :1097-1271 for one component from its edges' unique-evidence counts (count[k] belongs to edge k): the removals are pushed to
// rm in the reference's order, the return value is keep_component.
bool decide(const node_pair_t* edges, const uint32_t* count, uint32_t n, uint64_t V, int min_evidence, bool diploid_and_typical, std::vector<node_pair_t>& rm);

// The chain of :163-204 over the components in order, with the neighbour sets of :93-127.  count_component(i, min_evidence, rm) is
// countUniqueEvidence for component i: it pushes its removals and returns keep (or throws std::string with what the reference ends on).
// Fills outcome and min_evidence of every component and appends to c.to_remove.
void run_chain(Components& c, const hc_br_reduce_settings* st, const std::vector<int32_t>& min_evidence, const std::vector<uint8_t>& found,
               const std::function<bool(uint32_t, int, std::vector<node_pair_t>&)>& count_component);

// :206-207
void finish_removals(Components& c);

// evidence_per_edge as the tables hold it, with the pop_front of :1088 as a cursor per row
struct Evidence {
    const uint32_t* ev_edge;
    const uint64_t* ev_off;
    const uint32_t* ev_ids;
    uint64_t n_rows;
    std::vector<uint64_t> front;  // per row: the ids before it are popped
    Evidence(const uint32_t* e, const uint64_t* o, const uint32_t* i, uint64_t n) : ev_edge(e), ev_off(o), ev_ids(i), n_rows(n), front(o, o + n) {}
    int64_t row_of(node_id_t u, node_id_t v) const;  // -1: evidence_per_edge has no such key
};
// countUniqueEvidence's filter (:1014-1096) for one component on the lists themselves: count[k] = unique_evidence_per_edge's list length of
// edge k; consumes the lists.  *no_row: an edge had no key (:1029).  Throws std::string where the reference ends (include/hcsr.h).
void count_unique(Evidence& ev, const node_pair_t* edges, uint32_t n, uint32_t* count, bool* no_row);

void fill_counts(const Components& c, hc_br_reduce_counts* counts);

}  // namespace brr
}  // namespace hc
