// hc_api_sr_edge.cpp — the edge merge on the context's graph (include/hcsr.h): SRBuilder::mergeAlongEdges (reference
// src/SRBuilder.cpp:1238-1253) between the cleaned graph and consensus().
// hc_graph_merge_pairs: OverlapGraph::getEdgesForMerging (src/GraphAlgos.cpp:112-148) — the device packs the target column, the host walks.
// hc_sr_edge_merge: constructSuperread's ordering (src/SRBuilder.cpp:658-698), sort_vertices (:33-285) and calcSubreadInfo (:536-595) by the
// kernels of hc_sr_edge_kernels.hip, with hc_sr_consensus' own code (hc_api_sr.cpp: sr_consensus_run) in between.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

static const char* const kTied =
    ": the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first";

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" int hc_graph_merge_pairs(hc_ctx* c, uint32_t* pairs, uint64_t cap, uint64_t* n_pairs, hc_merge_pairs_stats* stats) {
    if (!c || !n_pairs) return fail(HC_ERR_ARG, "hc_graph_merge_pairs: null argument");
    if (stats) memset(stats, 0, sizeof *stats);
    *n_pairs = 0;
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_merge_pairs: no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, std::string("hc_graph_merge_pairs") + kTied);
    HC_HIP(hipSetDevice(c->device));
    const uint64_t V = g.n_vertices, E = g.n_edges;
    hipStream_t s = c->stream;
    int rc;
    if ((rc = c->sr_edge.targets.ensure((E ? E : 1) * sizeof(uint32_t)))) return rc;
    float ms_kernel = 0;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_edge_launch_targets(g.edges_out.as<hc_edge_rec>(), E, c->sr_edge.targets.as<uint32_t>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_kernel, c->ev0, c->ev1));
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> tgt(E);
    std::vector<uint64_t> off(V + 1);
    if (E) HC_HIP(hipMemcpyAsync(tgt.data(), c->sr_edge.targets.p, E * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(off.data(), g.out_off.p, (V + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    const double ms_copy = ms_since(t0);
    // getEdgesForMerging (src/GraphAlgos.cpp:112-148) on the packed column; the mirror (host/SrConsensus.cpp) walks the records
    t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> marked(V, 0);
    std::vector<uint32_t> taken;
    for (uint64_t v = 0; v < V; v++) {
        if (marked[v]) continue;
        for (uint64_t k = off[v]; k < off[v + 1]; k++) {
            const uint32_t w = tgt[k];  // (< V: hc_graph_load and hc_graph_resolve check the records)
            if (marked[w]) continue;
            taken.push_back((uint32_t)v);
            taken.push_back(w);
            marked[v] = marked[w] = 1;
            break;
        }
    }
    *n_pairs = taken.size() / 2;
    if (stats) {
        stats->ms_kernel = ms_kernel;
        stats->ms_copy = ms_copy;
        stats->ms_walk = ms_since(t0);
    }
    if (*n_pairs > cap || (*n_pairs && !pairs))
        return fail(HC_ERR_ARG, "hc_graph_merge_pairs: room for " + std::to_string(cap) + " pairs, " + std::to_string(*n_pairs) + " needed (*n_pairs)");
    if (*n_pairs) memcpy(pairs, taken.data(), taken.size() * sizeof(uint32_t));
    return HC_OK;
}

extern "C" int hc_sr_edge_merge(hc_ctx* c, const uint32_t* pairs, uint64_t n_pairs, const uint32_t* vertex_read, const uint8_t* vertex_fwd,
                                uint64_t n_vertices, const hc_sr_settings* settings, uint32_t* pair_status, uint64_t* first_layout,
                                hc_sr_layout* layouts, hc_sr_member* members, hc_sr_subread_info* subreads, int32_t* ret, uint32_t* status,
                                uint64_t* out_off, uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats) {
    const char* me = "hc_sr_edge_merge";
    if (!c || !settings || !first_layout || !out_off || !n_bytes || (n_vertices && (!vertex_read || !vertex_fwd)) ||
        (n_pairs && (!pairs || !pair_status || !layouts || !members || !subreads || !ret || !status)))
        return fail(HC_ERR_ARG, std::string(me) + ": null argument");
    if (!c->have_reads) return fail(HC_ERR_STATE, std::string(me) + ": hc_set_reads first");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, std::string(me) + ": no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, std::string(me) + kTied);
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, std::string(me) + ": min_qual is NaN");
    if (settings->min_clique_size == 0)
        return fail(HC_ERR_ARG, std::string(me) + ": min_clique_size == 0 sends a two-vertex clique through filter_subreads (src/SRBuilder.cpp:721), "
                                                  "which is not built");
    if (n_vertices != g.n_vertices) return fail(HC_ERR_ARG, std::string(me) + ": n_vertices is not the graph's");
    if (n_pairs >= (1ull << 31) - 1) return fail(HC_ERR_ARG, std::string(me) + ": more than 2^31 - 2 pairs");
    hc::sr_consensus_begin(c, out_off, n_bytes, stats);
    first_layout[0] = 0;
    if (n_pairs == 0) return hc::sr_consensus_run(c, me, 0, 0, settings, ret, status, out_off, cons_seq, cons_qual, cap, n_bytes, stats, nullptr);
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::SrEdge& W = c->sr_edge;
    const uint64_t V = n_vertices, n = n_pairs;
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n + 1, sizeof(uint64_t));
    int rc;
    if ((rc = W.pairs.ensure(2 * n * sizeof(uint32_t))) || (rc = W.vread.ensure((V ? V : 1) * sizeof(uint32_t))) || (rc = W.vfwd.ensure(V ? V : 1)) ||
        (rc = W.status.ensure(n * sizeof(uint32_t))) || (rc = W.lay_cnt.ensure((n + 1) * sizeof(uint64_t))) ||
        (rc = W.mem_cnt.ensure((n + 1) * sizeof(uint64_t))) || (rc = W.first.ensure((n + 1) * sizeof(uint64_t))) ||
        (rc = W.mem_off.ensure((n + 1) * sizeof(uint64_t))) || (rc = W.layouts.ensure(2 * n * sizeof(hc_sr_layout))) ||
        (rc = W.members.ensure(6 * n * sizeof(hc_sr_member))) || (rc = W.who.ensure(6 * n)) || (rc = W.sub.ensure(2 * n * sizeof(hc_sr_subread_info))) ||
        (rc = W.temp.ensure(scan_bytes ? scan_bytes : 16)))
        return rc;
    hipStream_t s = c->stream;
    HC_HIP(hipMemcpyAsync(W.pairs.p, pairs, 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (V) {
        HC_HIP(hipMemcpyAsync(W.vread.p, vertex_read, V * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(W.vfwd.p, vertex_fwd, V, hipMemcpyHostToDevice, s));
    }
    const hc::SrEdgeSlots slots{W.status.as<uint32_t>(), W.lay_cnt.as<uint64_t>(),     W.mem_cnt.as<uint64_t>(),
                                W.layouts.as<hc_sr_layout>(), W.members.as<hc_sr_member>(), W.who.as<uint8_t>()};
    float ms_lay = 0, ms_compact = 0, ms_sub = 0;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_edge_launch_layouts(c->view, g.edges_out.as<hc_edge_rec>(), g.out_off.as<unsigned long long>(), V, W.pairs.as<uint32_t>(), n,
                                      W.vread.as<uint32_t>(), W.vfwd.as<uint8_t>(), slots, s));
    HC_HIP(hc::prims::exclusive_sum(W.temp.p, W.temp.cap, W.lay_cnt.as<uint64_t>(), W.first.as<uint64_t>(), n + 1, s));
    HC_HIP(hc::prims::exclusive_sum(W.temp.p, W.temp.cap, W.mem_cnt.as<uint64_t>(), W.mem_off.as<uint64_t>(), n + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t n_members = 0;
    HC_HIP(hipMemcpyAsync(first_layout, W.first.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&n_members, W.mem_off.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(pair_status, W.status.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_lay, c->ev0, c->ev1));
    const uint64_t n_layouts = first_layout[n];
    if (n_layouts) {
        if ((rc = hc::sr_consensus_room(c, settings, n_layouts, n_members))) return rc;
        hc_ctx::Sr& S = c->sr;
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::sr_edge_launch_compact(slots, n, W.first.as<uint64_t>(), W.mem_off.as<uint64_t>(), S.layouts.as<hc_sr_layout>(),
                                          S.members.as<hc_sr_member>(), s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(layouts, S.layouts.p, n_layouts * sizeof(hc_sr_layout), hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(members, S.members.p, n_members * sizeof(hc_sr_member), hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms_compact, c->ev0, c->ev1));
    }
    bool ret_late = false;
    const int rc_run = hc::sr_consensus_run(c, me, n_layouts, n_members, settings, ret, status, out_off, cons_seq, cons_qual, cap, n_bytes, stats, &ret_late);
    // (HC_ERR_ARG here is the room of cons_seq / cons_qual: everything but the bytes is filled, the subread infos included)
    if (rc_run != HC_OK && rc_run != HC_ERR_ARG) return rc_run;
    if (n_layouts && ret_late) {  // a layout failed late: its ret is the host's
        std::vector<hc::SrLayoutInfo> info(n_layouts);
        for (uint64_t l = 0; l < n_layouts; l++) info[l] = hc::SrLayoutInfo{ret[l], status[l], 0, 0};
        HC_HIP(hipMemcpyAsync(c->sr.info.p, info.data(), n_layouts * sizeof(hc::SrLayoutInfo), hipMemcpyHostToDevice, s));
        HC_HIP(hipStreamSynchronize(s));  // (the host vector goes out of scope)
    }
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_edge_launch_subreads(slots, n, W.first.as<uint64_t>(), c->sr.info.as<hc::SrLayoutInfo>(), W.sub.as<hc_sr_subread_info>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipMemcpyAsync(subreads, W.sub.p, 2 * n * sizeof(hc_sr_subread_info), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_sub, c->ev0, c->ev1));
    if (stats) stats->ms_device += (double)ms_lay + ms_compact + ms_sub;
    return rc_run;
}
