// hc_cycles.h — launch interface of hc_cycles_kernels.hip: what surrounds the host's walk in hc_graph_remove_cycles (include/hcedge.h,
// "the second sortEdges and cycleRemovalHeuristic on the device graph") and the two small kernels of hc_graph_sort_edges.  The order:
// prepare, [host: ranked or sorted columns], first_try, [host: walk], components, [host: flagged vertices], compact, [host: permutation table], columns, [host: 19 walks, the best
// try], find_records, then hc::graph_remove_records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"
#include "hc_trans.h"

namespace hc {
namespace cycles {

enum Counter : uint32_t {
    kNanPlace,      // first place (vertex << 32 | position) of a record with a NaN score / mismatch_rate; kNoPlace: none
    kBadRead,       // hc_graph_sort_edges: records whose read1 / read2 is not below n_reads
    kComponents,    // flagged components
    kSubVertices,   // select's count
    kMissing,       // pairs without a record or an in-entry (cannot happen on a consistent graph)
    kTied,          // hc_graph_sort_edges: select's count of tied lists
    kLongList,      // the longest out-list, where it is longer than kRankMax (0: none is)
    kCounters = 8
};
constexpr unsigned long long kNoPlace = ~0ull;
constexpr uint32_t kSubColumns = 19;  // tries 2 .. 20
// A target column is ranked inside lists (a lane per record reads its own list: the sum of the squared list lengths) while no list is
// longer than this; a graph with a longer list takes three stable radix sorts per column instead (target, key, source).
constexpr uint32_t kRankMax = 1024;

// Device arrays of one hc_graph_remove_cycles for V vertices and E records (the caller carves them; sizes in elements).
struct Work {
    uint32_t *src, *tgt;                 // E: vertex1 / vertex2 of the records
    unsigned long long* key;             // E: try 1's key of the records
    uint32_t* col1;                      // E: try 1's target column
    unsigned long long *rk_a, *rk_b;     // V: in-degree << 32 | vertex, unsorted and sorted
    uint32_t* parent;                    // V: union-find, then every vertex's root
    uint8_t *root_flag, *vflag;          // V: the root owns a pair of try 1; the vertex lies under such a root
    uint32_t *sub_vtx, *lid;             // V: the flagged vertices ascending; their index in that list
    unsigned long long *sub_off, *perm_base;  // V + 1: the compact CSR's offsets; V: where a vertex's 16 permutations start in `table`
    uint32_t *sub_src, *sub_tgt;         // E: the compact CSR's owner and target (renumbered), list order
    unsigned long long* sub_key;         // 3 E: the keys of tries 2, 3, 4, one column each
    uint32_t* cols;                      // 19 E: the target columns of tries 2 .. 20, n_sub_edges apart
    uint32_t* table;                     // 16 E at most: the permutations by distinct list length (host-built)
    uint32_t* pair_u;                    // E: the sources of try 1's pairs
    unsigned long long* pairs;           // E: the applied pairs u << 32 | v
    uint32_t *rec, *in_pos;              // E: their first record and first in-entry
    // the radix form of a column (graphs with a list longer than kRankMax), carved only then: keys and record indices, in and out
    uint32_t *rs_k32a, *rs_k32b, *rs_idx_a, *rs_idx_b;  // E
    unsigned long long *rs_k64a, *rs_k64b;              // E
    unsigned long long* counters;        // kCounters
    void* temp;                          // the prims' workspace
    size_t temp_bytes;
};

size_t temp_bytes(uint64_t E, uint64_t V);
// the counters' start values and kLongList
hipError_t prepare(const trans::Graph& g, const Work& w, hipStream_t s);
// src / tgt / try 1's column (radix: by the three sorts), the roots' keys sorted (rk_b), the NaN place
hipError_t first_try(const trans::Graph& g, const Work& w, bool radix, hipStream_t s);
// weak components; the vertices under the roots of pair_u[0 .. n_pairs) flagged and selected (counters: kComponents, kSubVertices)
hipError_t components(const trans::Graph& g, const Work& w, uint32_t n_pairs, hipStream_t s);
// the compact CSR's frame for the n_sub flagged vertices: lid, sub_off (n_sub + 1)
hipError_t compact(const trans::Graph& g, const Work& w, uint32_t n_sub, hipStream_t s);
// its lists (sub_src / sub_tgt, the keys of tries 2 - 4) and cols: tries 2 - 4 ranked by key, tries 5 - 20 gathered through table /
// perm_base (on the device already)
hipError_t columns(const trans::Graph& g, const Work& w, uint32_t n_sub, uint64_t n_sub_edges, bool radix, hipStream_t s);
// rec / in_pos of pairs[0 .. n) (counters: kMissing)
hipError_t find_records(const trans::Graph& g, const Work& w, uint32_t n, hipStream_t s);

// hc_graph_sort_edges: idx = 0, 1, ..., the records naming a read >= n_reads counted into *bad; seq_out[k] = seq[order[k]]
hipError_t sort_prepare(const trans::Graph& g, uint32_t* idx, uint64_t n_reads, unsigned long long* bad, hipStream_t s);
hipError_t gather_seq(const uint32_t* seq, const uint32_t* order, uint32_t n, uint32_t* seq_out, hipStream_t s);

}  // namespace cycles
}  // namespace hc
