// hc_api_graph_text.cpp — hc_graph_write_text and hc_graph_text_fetch (include/hcedge.h): graph.txt, digraph.txt and the GFA files of
// the graph the context holds, as bytes on the device.  Decide (hc_graph_text_kernels.hip), one exclusive sum over the items' byte
// counts (hc_prims.hip), the counters and the total back to the host — which sizes the text block and refuses a failed assert —, write.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/hcedge.h"
#include "hc_ctx.h"
#include "hc_graph_text.h"
#include "hc_prims.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

extern "C" {

int hc_graph_write_text(hc_ctx* c, uint32_t kind, const hc_graph_text_settings* st, hc_graph_text_counts* counts) {
    const char* me = "hc_graph_write_text: ";
    if (!c || !st || !counts) return fail(HC_ERR_ARG, std::string(me) + "null argument");
    memset(counts, 0, sizeof *counts);
    if (kind > HC_GRAPH_TEXT_GFA) return fail(HC_ERR_ARG, std::string(me) + "unknown kind");
    hc_ctx::Graph& g = c->graph;
    hc_ctx::GraphText& T = c->graph_text;
    T.valid = false;
    T.n_bytes = 0;
    if (!g.valid) return fail(HC_ERR_STATE, std::string(me) + "no graph on the device");
    if (g.n_tied)
        return fail(HC_ERR_STATE, std::string(me) + "the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): "
                                                    "hc_graph_load the host's lists first");
    hc::gtext::Reads reads{nullptr, nullptr, nullptr, 0, 0};
    if (kind == HC_GRAPH_TEXT_GFA) {
        const hc_ctx::SrNext& N = c->srn;
        if (!N.raw_valid || N.h_first.empty()) return fail(HC_ERR_STATE, std::string(me) + "GFA needs the raw arrays of the store (hc_sr_keep_device, then hc_set_reads)");
        const uint64_t n_reads = N.h_first.size() - 1;
        if (st->n_singles > n_reads) return fail(HC_ERR_ARG, std::string(me) + "n_singles exceeds the reads of the store");
        reads = hc::gtext::Reads{N.bases.as<uint8_t>(), N.off.as<uint64_t>(), N.first.as<uint32_t>(), (uint32_t)n_reads, (uint32_t)st->n_singles};
    }
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t V = g.n_vertices, E = g.n_edges, n_items = hc::gtext::n_items(kind, V, E);  // (V, E < 2^31: n_items + 1 < 2^32, the scan's limit)
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n_items + 1, sizeof(uint64_t));
    int rc;
    if ((rc = T.sizes.ensure((n_items + 1) * sizeof(uint64_t))) || (rc = T.keep.ensure(E ? E : 1)) ||
        (rc = T.counters.ensure(hc::gtext::kCounters * sizeof(unsigned long long))) || (rc = T.temp.ensure(scan_bytes)))
        return rc;
    const hc::gtext::Graph view{g.edges_out.as<hc_edge_rec>(), g.out_off.as<unsigned long long>(), g.incl.as<uint8_t>(), (uint32_t)V, (uint32_t)E};
    unsigned long long* d_counters = T.counters.as<unsigned long long>();
    uint64_t* d_sizes = T.sizes.as<uint64_t>();
    HC_HIP(hipMemsetAsync(d_counters, 0, hc::gtext::kCounters * sizeof(unsigned long long), s));
    HC_HIP(hipMemsetAsync(d_counters + hc::gtext::kKey, 0xff, sizeof(unsigned long long), s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::gtext::decide(kind, view, reads, st->edge_threshold, st->merge_contigs, d_sizes, T.keep.as<uint8_t>(), d_counters, s));
    HC_HIP(hc::prims::exclusive_sum(T.temp.p, T.temp.cap, d_sizes, d_sizes, n_items + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    unsigned long long h[hc::gtext::kCounters];
    uint64_t body = 0;
    HC_HIP(hipMemcpyAsync(h, d_counters, sizeof h, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&body, d_sizes + n_items, sizeof body, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    float ms = 0;
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device = ms;
    if (h[hc::gtext::kKey] != hc::gtext::kNoKey) {  // the reference would have stopped here
        const uint64_t key = h[hc::gtext::kKey], place = (key >> 2) & 0x7fffffffull;
        counts->status = hc::gtext::kStatus[kind][key & 3];
        counts->bad_v = key >> 33;
        counts->bad_pos = place ? place - 1 : 0;
        return HC_OK;
    }
    uint64_t header = 0;
    if (kind == HC_GRAPH_TEXT_CLIQUES) header = std::to_string(V).size() + std::to_string(2 * h[hc::gtext::kPairs]).size() + 2;
    if (kind == HC_GRAPH_TEXT_GFA) header = hc::gtext::kGfaHeaderBytes;
    const uint64_t n_bytes = header + body;
    if ((rc = T.text.ensure(n_bytes ? n_bytes : 1))) return rc;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::gtext::write(kind, view, reads, d_sizes, T.keep.as<uint8_t>(), d_counters, T.text.as<char>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device += ms;
    counts->n_bytes = n_bytes;
    counts->n_pairs = h[hc::gtext::kPairs];
    counts->n_segments = h[hc::gtext::kSegments];
    counts->l_count = h[hc::gtext::kLinks];
    counts->c_count = h[hc::gtext::kContained];
    counts->n_lines = kind == HC_GRAPH_TEXT_CLIQUES ? 2 + 2 * counts->n_pairs
                      : kind == HC_GRAPH_TEXT_DIGRAPH ? E
                                                      : 1 + counts->n_segments + counts->l_count + counts->c_count;
    T.n_bytes = n_bytes;
    T.valid = true;
    return HC_OK;
}

int hc_graph_text_fetch(hc_ctx* c, uint64_t first, uint64_t count, char* dst) {
    if (!c) return fail(HC_ERR_ARG, "hc_graph_text_fetch: null context");
    const hc_ctx::GraphText& T = c->graph_text;
    if (!T.valid) return fail(HC_ERR_STATE, "hc_graph_text_fetch: no text on the device (hc_graph_write_text first)");
    if (first > T.n_bytes || count > T.n_bytes - first) return fail(HC_ERR_ARG, "hc_graph_text_fetch: range beyond the text");
    if (count == 0) return HC_OK;
    if (!dst) return fail(HC_ERR_ARG, "hc_graph_text_fetch: null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, T.text.as<char>() + first, count, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

}  // extern "C"
