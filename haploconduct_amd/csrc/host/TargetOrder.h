// TargetOrder.h — std::sort's order of an out-list by target, shared by the host mirror of removeTransitiveEdges
// (host_model.cpp) and the device route, which hands the lists where it can differ from a stable sort to the host
// (hc_api_stage.cpp via hc_trans_kernels.hip).  Plain C++: the host files also build without HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace hc {

// OverlapGraph::sortAdjOut (src/GraphAlgos.cpp:806-833) sorts one out-list with std::sort and a comparator on the
// target only.  std::sort's result depends on the comparisons alone, so the same call over (target, position) pairs
// gives the same permutation: perm[k] = the position (in the list as it was) of the k-th entry afterwards.
inline void target_sort_perm(const uint32_t* targets, size_t n, uint32_t* perm) {
    std::vector<std::pair<uint32_t, uint32_t>> pairs(n);
    for (size_t k = 0; k < n; k++) pairs[k] = std::make_pair(targets[k], (uint32_t)k);
    std::sort(pairs.begin(), pairs.end(),
              [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
    for (size_t k = 0; k < n; k++) perm[k] = pairs[k].second;
}

}  // namespace hc
