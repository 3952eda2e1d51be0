// hc_graph_text.h — what the kernels (hc_graph_text_kernels.hip) and the glue (hc_api_graph_text.cpp) of hc_graph_write_text
// (include/hcedge.h) share: the layout of the items, the packed key of a failed assert, the counters and the launch interface.
//
// Items in file order.  CLIQUES and DIGRAPH: item k = record k.  GFA: the item of vertex i sits at out_off[i] + i, the item of
// record k of its list at k + i + 1, V + E items.  sizes[] holds n_items + 1 byte counts (the last 0); its exclusive sum places every
// item behind the header, whose length the write pass knows (CLIQUES: from the pair count).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"

namespace hc {
namespace gtext {

// The first failed assert in file order: atomicMin over vertex << 33 | place << 2 | code; place = 0 for a status of the vertex
// itself, list position + 1 for one of a record (V, E < 2^31).  A kind has at most four statuses: code indexes kStatus[kind].
constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kStatus[3][4] = {
    {HC_GRAPH_TEXT_SELF_LOOP, HC_GRAPH_TEXT_INCLUSION_HAS_EDGES, HC_GRAPH_TEXT_WEAK_EDGE, 0u},
    {HC_GRAPH_TEXT_SELF_LOOP, 0u, 0u, 0u},
    {HC_GRAPH_TEXT_SELF_LOOP, HC_GRAPH_TEXT_PAIRED_IN_SINGLES, HC_GRAPH_TEXT_EMPTY_SEQ, HC_GRAPH_TEXT_BAD_BASE}};
__host__ __device__ inline uint64_t bad_key(uint32_t v, uint32_t place, uint32_t code) { return (uint64_t)v << 33 | (uint64_t)place << 2 | code; }

// counters[]: the key above, then the tallies (one atomic per workgroup)
enum { kKey = 0, kPairs = 1, kSegments = 2, kLinks = 3, kContained = 4, kCounters = 8 };
constexpr uint32_t kGfaHeaderBytes = 11;  // "H\tVN:Z:1.0\n"

struct Graph {
    const hc_edge_rec* E;
    const unsigned long long* out_off;  // V + 1
    const uint8_t* incl;                // V
    uint32_t V, n_edges;
};
struct Reads {  // the raw arrays hc_sr_keep_device keeps: bytes, seq_off (n_seq + 1), read_first_seq (n_reads + 1)
    const uint8_t* bases;
    const uint64_t* off;
    const uint32_t* first;
    uint32_t n_reads, n_singles;
};

__host__ __device__ inline uint64_t n_items(uint32_t kind, uint64_t V, uint64_t E) { return kind == HC_GRAPH_TEXT_GFA ? V + E : E; }

// Decide: sizes[0 .. n_items] (the last 0), keep[0 .. E), the counters (zeroed / kNoKey by the call).  Two launches for GFA
// (vertices, records), one otherwise.
hipError_t decide(uint32_t kind, const Graph& g, const Reads& r, double edge_threshold, double merge_contigs, uint64_t* sizes, uint8_t* keep,
                  unsigned long long* counters, hipStream_t stream);
// Write: place[] = the exclusive sum of sizes[]; text has room for header + place[n_items] bytes.  Two launches for GFA (record
// lines and header, segment lines), one otherwise.
hipError_t write(uint32_t kind, const Graph& g, const Reads& r, const uint64_t* place, const uint8_t* keep, const unsigned long long* counters,
                 char* text, hipStream_t stream);

}  // namespace gtext
}  // namespace hc
