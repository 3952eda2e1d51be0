// SrCliqueFilter.h — the rule by which filter_subreads' selection (reference src/SRBuilder.cpp:597-622) is decided without knowing how
// sortVerticesByEndpos' unstable std::sort (:640) orders entries of equal endpos.  For host and device: the mirror (host/SrClique.cpp)
// and sr_clique_filter_kernel (hc_sr_clique_kernels.hip) take it from here, so that the two cannot drift.  Plain C++ that also
// compiles as device code.
//
// The reference selects the distinct vertices of the first num / 2 list entries and the base (:603-605), then walks the entries from the
// largest endpos down and adds vertices until `num` are selected (:617-622).  Seen per GROUP of equal endpos, with g = the group's distinct
// vertices that are not selected yet and need = num - |selected|:
//   g <= need   the whole group is taken whatever its inner order: the set does not depend on the sort;
//   need == 0   the walk is over;
//   need < g    the group is CUT: which of its vertices are taken depends on the order among ties.  In a layout of at most 16 entries
//               libstdc++'s std::sort is a single insertion sort (introsort's threshold, _S_threshold = 16), which is stable, so the
//               walk from the back meets the group's entries in reversed list order.  A longer layout goes to std::sort itself.
#pragma once
#include <stdint.h>

#include "../../../include/hcsr.h"
#include "SrCodes.h"

namespace hc {
namespace srclique {

constexpr uint32_t kStableSortMax = 16;  // std::sort on at most this many elements is one insertion sort

enum GroupStep : uint32_t { kTakeGroup = 0, kCutStable = 1, kCutHost = 2 };

// what to do with a group of g not yet selected distinct vertices when `need` (> 0) are still wanted, in a layout of n_entries
HC_SR_HD inline GroupStep group_step(uint32_t g, uint32_t need, uint32_t n_entries) {
    if (g <= need) return kTakeGroup;
    return n_entries <= kStableSortMax ? kCutStable : kCutHost;
}

// HC_SR_FILTER_* of a layout whose walk met `step` last
HC_SR_HD inline uint32_t filter_class(GroupStep step) {
    return step == kTakeGroup ? HC_SR_FILTER_GROUPS : step == kCutStable ? HC_SR_FILTER_STABLE : HC_SR_FILTER_HOST;
}

// does a clique of this size go through filter_subreads (:721), and with which num (:725)
HC_SR_HD inline bool is_filtered(uint64_t clique_size, uint32_t min_clique_size) { return clique_size > 3ull * min_clique_size; }
HC_SR_HD inline uint32_t filter_num(uint32_t min_clique_size) { return 2u * min_clique_size; }

}  // namespace srclique
}  // namespace hc
