// hc_label.h — launch interface of hc_label_kernels.hip: OverlapGraph::vertexLabellingHeuristic + checkDuplicateEdges on the device graph
// (include/hcedge.h, "vertex labelling on the device graph").  The order: prepare, [host: refusal], components, [host: the tries of the
// inconsistent components, host/Labelling.h], conflicts, [host: the best try], apply, check_duplicates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"
#include "hc_trans.h"

namespace hc {
namespace label {

enum Counter : uint32_t {
    kRepeated,     // first place (vertex << 32 | position) of a record that repeats an earlier one of its list; kNoPlace: none
    kDuplicate,    // first place of checkDuplicateEdges' assert; kNoPlace: none
    kComponents,
    kInconsistent,
    kHostVertices,  // select's count
    kMoved,
    kDeleted,
    kSwitched,
    kTry0,  // conflicts of try t at kTry0 + t - 1
    kCounters = kTry0 + 100
};
constexpr unsigned long long kNoPlace = ~0ull;

// Device arrays of one call for V vertices and E records (the caller carves them; sizes in elements).
struct Work {
    uint32_t *src, *tgt;                            // E: vertex1 / vertex2 of the records on entry
    uint8_t* same;                                  // E: ori1 == ori2 (a record keeps it through every switch)
    uint32_t* parent;                               // 2 V: union-find over "vertex with parity", then every element's root
    unsigned long long* start;                      // 2 V: per root slot, min of in-degree << 32 | vertex over the component
    unsigned long long* L;                          // 2 V: bit t - 1 of L[2 v] (tries 1 - 64) / L[2 v + 1] (65 - 100): label of v at try t
    uint8_t* host_flag;                             // V: the vertex lies in a component with an odd cycle
    uint32_t *host_vtx, *lid;                       // V: those vertices ascending; their index in that list
    unsigned long long *sub_in_off, *sub_out_off;   // V + 1: the compact subgraph of host/Labelling.h
    uint32_t *sub_in, *sub_out;                     // E
    uint8_t* sub_same;                              // E
    unsigned long long* bits;                       // 2 V: label_tries' result, by host_vtx index
    uint8_t* rec_flag;                              // E: kKeep / kMove / kDelete at the best try
    uint32_t *mv_sum, *keep_sum;                    // E + 1: moved records / kept in-entries, flags and then their exclusive sums
    uint32_t *in_owner, *rm_in;                     // E: the vertex an in-entry belongs to; V: records towards the vertex that leave
    unsigned long long *keys_a, *keys_b;            // E
    uint32_t *val_a, *val_b;                        // E
    uint8_t* orient;                                // V
    unsigned long long* counters;                   // kCounters
    void* temp;                                     // the prims' workspace
    size_t temp_bytes;
};
enum : uint8_t { kKeep = 0, kMove = 1, kDelete = 2 };

size_t temp_bytes(uint64_t E, uint64_t V);
// src / tgt / same, the repeated-record check and the counters' start values
hipError_t prepare(const trans::Graph& g, const Work& w, hipStream_t s);
// components with parity, start vertices, the labels of the consistent components, host_flag / host_vtx (counters: kComponents,
// kInconsistent, kHostVertices)
hipError_t components(const trans::Graph& g, const Work& w, hipStream_t s);
// the compact subgraph of the n_host flagged vertices: sub_in_off / sub_out_off (n_host + 1), sub_in / sub_out / sub_same
hipError_t compact_subgraph(const trans::Graph& g, const Work& w, uint32_t n_host, hipStream_t s);
// w.bits (2 n_host words, on the device) into L
hipError_t scatter_bits(const Work& w, uint32_t n_host, hipStream_t s);
// conflicts per try into counters[kTry0 ..]
hipError_t conflicts(const trans::Graph& g, const Work& w, uint32_t n_tries, hipStream_t s);
// replay, rebuild into `out` (out.E is not set: the caller reads kDeleted), orientations of try best (0-based)
hipError_t apply(const trans::Graph& g, trans::Graph& out, const Work& w, uint32_t n_tries, uint32_t best, hipStream_t s);
// checkDuplicateEdges on g into counters[kDuplicate] (reset here)
hipError_t check_duplicates(const trans::Graph& g, const Work& w, hipStream_t s);

}  // namespace label
}  // namespace hc
