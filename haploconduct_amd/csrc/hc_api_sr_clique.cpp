// hc_api_sr_clique.cpp — cliques of any size on the context's graph (include/hcsr.h: hc_sr_clique_merge): constructSuperread (reference
// src/SRBuilder.cpp:654-748) by the kernels of hc_sr_clique_kernels.hip, three stable radix sorts and the exclusive sums of hc_prims.h, with
// hc_sr_consensus' own code (hc_api_sr.cpp: sr_consensus_room / sr_consensus_run) on the USED members.  A filter that cuts a group of equal
// endpos in a layout of more than 16 entries is decided here on the host, by the mirror's own function (hc_host_sr_clique_filter): the
// pattern of the consensus' host-finished columns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int bits_for(uint64_t n) {  // bits that hold every value below n
    int b = 1;
    while (b < 32 && (1ull << b) < n) b++;
    return b;
}

extern "C" int hc_sr_clique_filter_on_host(hc_ctx* c, int on) {
    if (!c) return fail(HC_ERR_ARG, "hc_sr_clique_filter_on_host: null argument");
    c->sr_clique.filter_on_host = on != 0;
    return HC_OK;
}

extern "C" int hc_sr_clique_merge(hc_ctx* c, const uint64_t* clique_off, const uint32_t* clique_nodes, uint64_t n_cliques, const uint32_t* vertex_read,
                                  const uint8_t* vertex_fwd, uint64_t n_vertices, const hc_sr_settings* settings, uint32_t* clique_status,
                                  uint64_t* first_layout, hc_sr_layout* layouts, hc_sr_member* members, uint32_t* member_vertex, uint8_t* member_used,
                                  uint8_t* layout_filter, hc_sr_subread_info* subreads, int32_t* ret, uint32_t* status, uint64_t* out_off,
                                  uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_clique_stats* stats) {
    const std::string me = "hc_sr_clique_merge";
    if (stats) memset(stats, 0, sizeof *stats);
    if (!c || !settings || !first_layout || !out_off || !n_bytes || !clique_off || (n_vertices && (!vertex_read || !vertex_fwd)) ||
        (n_cliques && (!clique_status || !layouts || !ret || !status)))
        return fail(HC_ERR_ARG, me + ": null argument");
    if (!c->have_reads) return fail(HC_ERR_STATE, me + ": hc_set_reads first");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, me + ": no graph on the device");
    if (g.n_tied)
        return fail(HC_ERR_STATE, me + ": the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the "
                                       "host's lists first");
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, me + ": min_qual is NaN");
    if (settings->min_clique_size == 0)
        return fail(HC_ERR_ARG, me + ": min_clique_size == 0: filter_subreads (src/SRBuilder.cpp:725) is then called with num == 0 and may drop the "
                                     "first list entry, a layout the consensus refuses");
    if (n_vertices != g.n_vertices) return fail(HC_ERR_ARG, me + ": n_vertices is not the graph's");
    if (n_cliques >= (1ull << 31) - 1 || settings->min_clique_size >= (1u << 30)) return fail(HC_ERR_ARG, me + ": more than 2^31 - 2 cliques");
    if (clique_off[0] != 0) return fail(HC_ERR_ARG, me + ": clique_off[0] is not 0");
    for (uint64_t i = 0; i < n_cliques; i++)
        if (clique_off[i + 1] < clique_off[i]) return fail(HC_ERR_ARG, me + ": clique_off descends");
    const uint64_t C = n_cliques, N = clique_off[C], V = n_vertices;
    if (N >= (1ull << 31) || g.n_edges >= (1ull << 32)) return fail(HC_ERR_ARG, me + ": 2^31 clique entries or 2^32 records or more");
    if (N && (!clique_nodes || !members || !member_vertex || !member_used || !subreads)) return fail(HC_ERR_ARG, me + ": null argument");
    hc_sr_stats* sr_stats = stats ? &stats->sr : nullptr;
    hc::sr_consensus_begin(c, out_off, n_bytes, sr_stats);
    first_layout[0] = 0;
    if (C == 0) return hc::sr_consensus_run(c, me.c_str(), 0, 0, settings, ret, status, out_off, cons_seq, cons_qual, cap, n_bytes, sr_stats, nullptr);
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::SrClique& B = c->sr_clique;
    const uint64_t N1 = N ? N : 1, M2 = 2 * N1, C1 = C + 1;
    size_t temp_bytes = std::max(hc::prims::scan_temp_bytes(M2 + 1, sizeof(uint64_t)), hc::prims::scan_temp_bytes(C1, sizeof(uint64_t)));
    temp_bytes = std::max(temp_bytes, hc::prims::sort_temp_bytes(M2, sizeof(uint64_t), sizeof(uint32_t)));
    temp_bytes = std::max(temp_bytes, hc::prims::sort_temp_bytes(N1, sizeof(uint64_t), 0));
    int rc;
    if ((rc = B.off.ensure(C1 * 8)) || (rc = B.nodes.ensure(N1 * 4)) || (rc = B.vread.ensure((V ? V : 1) * 4)) || (rc = B.vfwd.ensure(V ? V : 1)) ||
        (rc = B.key_in.ensure(N1 * 8)) || (rc = B.key.ensure(N1 * 8)) || (rc = B.hit.ensure(N1 * 4)) || (rc = B.slot.ensure(N1 * sizeof(hc::SrCliqueSlot))) ||
        (rc = B.ecnt.ensure((N1 + 1) * 8)) || (rc = B.eoff.ensure((N1 + 1) * 8)) || (rc = B.sel.ensure(M2 * 4)) ||
        (rc = B.sub.ensure(N1 * sizeof(hc_sr_subread_info))) || (rc = B.failkey.ensure(C * 8)) || (rc = B.base_rank.ensure(C * 4)) ||
        (rc = B.type.ensure(C)) || (rc = B.geom.ensure(C * 4)) || (rc = B.ext.ensure(4 * C * 8)) || (rc = B.deg.ensure(C1 * 8)) ||
        (rc = B.rec_off.ensure(C1 * 8)) || (rc = B.lay0.ensure(C1 * 8)) || (rc = B.pl_first.ensure(C1 * 8)) || (rc = B.status.ensure(C * 4)) ||
        (rc = B.lay_cnt.ensure(C1 * 8)) || (rc = B.first.ensure(C1 * 8)) || (rc = B.mem_cnt.ensure(C1 * 8)) || (rc = B.mem_off.ensure(C1 * 8)) ||
        (rc = B.pl.ensure(2 * C * sizeof(hc::SrCliquePl))) || (rc = B.pl_total.ensure(2 * C * 4)) || (rc = B.pl_filter.ensure(2 * C)) ||
        (rc = B.ekey_in.ensure(M2 * 8)) || (rc = B.ekey.ensure(M2 * 8)) || (rc = B.eval_in.ensure(M2 * 4)) || (rc = B.eval.ensure(M2 * 4)) ||
        (rc = B.ekey2.ensure(M2 * 8)) || (rc = B.eval2.ensure(M2 * 4)) || (rc = B.slotpos.ensure(M2 * 4)) ||
        (rc = B.fmem.ensure(M2 * sizeof(hc_sr_member))) || (rc = B.fvert.ensure(M2 * 4)) || (rc = B.fend.ensure(M2 * 4)) || (rc = B.fused.ensure(M2)) ||
        (rc = B.out_layouts.ensure(2 * C * sizeof(hc_sr_layout))) || (rc = B.out_members.ensure(M2 * sizeof(hc_sr_member))) ||
        (rc = B.out_vertex.ensure(M2 * 4)) || (rc = B.out_used.ensure(M2)) || (rc = B.out_filter.ensure(2 * C)) || (rc = B.uflag.ensure((M2 + 1) * 8)) ||
        (rc = B.uoff.ensure((M2 + 1) * 8)) || (rc = B.temp.ensure(temp_bytes ? temp_bytes : 16)))
        return rc;
    hipStream_t s = c->stream;
    HC_HIP(hipMemcpyAsync(B.off.p, clique_off, C1 * 8, hipMemcpyHostToDevice, s));
    if (N) HC_HIP(hipMemcpyAsync(B.nodes.p, clique_nodes, N * 4, hipMemcpyHostToDevice, s));
    if (V) {
        HC_HIP(hipMemcpyAsync(B.vread.p, vertex_read, V * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(B.vfwd.p, vertex_fwd, V, hipMemcpyHostToDevice, s));
    }
    hc::SrCliqueView W{};
    W.C = C, W.N = N, W.V = V;
    W.off = B.off.as<uint64_t>(), W.vread = B.vread.as<uint32_t>(), W.vfwd = B.vfwd.as<uint8_t>();
    W.E = g.edges_out.as<hc_edge_rec>(), W.out_off = g.out_off.as<unsigned long long>(), W.m = settings->min_clique_size;
    W.key = B.key.as<uint64_t>(), W.hit = B.hit.as<uint32_t>(), W.slot = B.slot.as<hc::SrCliqueSlot>(), W.ecnt = B.ecnt.as<uint64_t>();
    W.eoff = B.eoff.as<uint64_t>(), W.sel = B.sel.as<uint32_t>(), W.sub = B.sub.as<hc_sr_subread_info>();
    W.failkey = B.failkey.as<unsigned long long>(), W.base_rank = B.base_rank.as<uint32_t>(), W.type = B.type.as<uint8_t>();
    W.geom = B.geom.as<uint32_t>(), W.ext = B.ext.as<unsigned long long>(), W.deg = B.deg.as<uint64_t>(), W.rec_off = B.rec_off.as<uint64_t>();
    W.lay0 = B.lay0.as<uint64_t>(), W.pl_first = B.pl_first.as<uint64_t>(), W.status = B.status.as<uint32_t>();
    W.lay_cnt = B.lay_cnt.as<uint64_t>(), W.first = B.first.as<uint64_t>(), W.mem_cnt = B.mem_cnt.as<uint64_t>(), W.mem_off = B.mem_off.as<uint64_t>();
    W.pl = B.pl.as<hc::SrCliquePl>(), W.pl_total = B.pl_total.as<int32_t>(), W.pl_filter = B.pl_filter.as<uint8_t>();
    W.ekey_in = B.ekey_in.as<uint64_t>(), W.ekey = B.ekey.as<uint64_t>(), W.eval_in = B.eval_in.as<uint32_t>(), W.eval = B.eval.as<uint32_t>();
    W.slotpos = B.slotpos.as<uint32_t>(), W.fmem = B.fmem.as<hc_sr_member>(), W.fvert = B.fvert.as<uint32_t>(), W.fend = B.fend.as<int32_t>();
    W.fused = B.fused.as<uint8_t>(), W.out_layouts = B.out_layouts.as<hc_sr_layout>(), W.out_members = B.out_members.as<hc_sr_member>();
    W.out_vertex = B.out_vertex.as<uint32_t>(), W.out_used = B.out_used.as<uint8_t>(), W.out_filter = B.out_filter.as<uint8_t>();
    W.uflag = B.uflag.as<uint64_t>(), W.uoff = B.uoff.as<uint64_t>();
    float ms = 0;
    double ms_layout = 0;
    // 1-3. the cliques' vertices in order, the range checks, type and base, the bases' lists
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_clique_launch_keys(W, B.nodes.as<uint32_t>(), B.key_in.as<uint64_t>(), s));
    if (N) HC_HIP(hc::prims::sort_keys(B.temp.p, B.temp.cap, B.key_in.as<uint64_t>(), W.key, N, 0, 32 + bits_for(C), s));
    HC_HIP(hc::sr_clique_launch_precheck(c->view, W, s));
    HC_HIP(hc::sr_clique_launch_bases(W, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.deg, W.rec_off, C1, s));
    HC_HIP(hipMemsetAsync(B.hit.p, 0xff, N1 * 4, s));
    HC_HIP(hipMemsetAsync(B.sel.p, 0, M2 * 4, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t n_records = 0;
    HC_HIP(hipMemcpyAsync(&n_records, W.rec_off + C, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_layout += ms;
    if (n_records >= (1ull << 32)) return fail(HC_ERR_ARG, me + ": the bases' lists hold 2^32 records or more");
    // 3-4. getEdgeInfo, the per-node part of the loop, the entries
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_clique_launch_hits(W, n_records, s));
    HC_HIP(hc::sr_clique_launch_nodes(c->view, W, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.ecnt, W.eoff, N + 1, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.lay0, W.pl_first, C1, s));
    HC_HIP(hc::sr_clique_launch_entries(W, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t n_entries = 0, n_pl = 0;
    HC_HIP(hipMemcpyAsync(&n_entries, W.eoff + N, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&n_pl, W.pl_first + C, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_layout += ms;
    if (n_entries > M2 || n_pl > 2 * C) return fail(HC_ERR_HIP, me + ": the entry count left its bound");
    // 4-6. the list order, the geometry, the endpos order, the filter
    const int pl_bits = bits_for(2 * C);
    HC_HIP(hipEventRecord(c->ev0, s));
    if (n_entries) {
        HC_HIP(hc::prims::sort_pairs(B.temp.p, B.temp.cap, W.ekey_in, W.ekey, W.eval_in, W.eval, n_entries, 0, 32 + pl_bits, s));
        HC_HIP(hc::sr_clique_launch_geometry(W, n_entries, s));
        HC_HIP(hc::prims::sort_pairs(B.temp.p, B.temp.cap, W.ekey_in, B.ekey2.as<uint64_t>(), W.eval_in, B.eval2.as<uint32_t>(), n_entries, 0,
                                     32 + pl_bits, s));
        HC_HIP(hc::sr_clique_launch_filter(W, n_pl, B.ekey2.as<uint64_t>(), B.eval2.as<uint32_t>(), s));
    }
    HC_HIP(hc::sr_clique_launch_status(W, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.lay_cnt, W.first, C1, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.mem_cnt, W.mem_off, C1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t n_members = 0;
    std::vector<uint8_t> pl_filter(n_pl);
    std::vector<hc::SrCliquePl> pls(n_pl);
    HC_HIP(hipMemcpyAsync(first_layout, W.first, C1 * 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&n_members, W.mem_off + C, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(clique_status, W.status, C * 4, hipMemcpyDeviceToHost, s));
    if (n_pl) {
        HC_HIP(hipMemcpyAsync(pl_filter.data(), W.pl_filter, n_pl, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(pls.data(), W.pl, n_pl * sizeof(hc::SrCliquePl), hipMemcpyDeviceToHost, s));
    }
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_layout += ms;
    const uint64_t n_layouts = first_layout[C];
    // 6. the filters the host decides: the layouts the device listed (all filtered ones under hc_sr_clique_filter_on_host)
    uint64_t n_filtered = 0, n_host_class = 0;
    std::vector<uint64_t> host_pl;
    for (uint64_t p = 0; p < n_pl; p++) {
        if (pl_filter[p] == HC_SR_FILTER_NONE) continue;
        n_filtered++;
        if (pl_filter[p] == HC_SR_FILTER_HOST) n_host_class++;
        if (pl_filter[p] == HC_SR_FILTER_HOST || B.filter_on_host) host_pl.push_back(p);
    }
    double ms_host_filter = 0;
    if (!host_pl.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> vert(n_entries);
        std::vector<int32_t> endpos(n_entries);
        std::vector<uint8_t> used(n_entries);
        std::vector<uint64_t> key(N);
        std::vector<uint32_t> base_rank(C);
        HC_HIP(hipMemcpyAsync(vert.data(), W.fvert, n_entries * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(endpos.data(), W.fend, n_entries * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(used.data(), W.fused, n_entries, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(key.data(), W.key, N * 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(base_rank.data(), W.base_rank, C * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        const uint32_t num = 2 * settings->min_clique_size;
        std::atomic<uint64_t> next{0};
        std::atomic<int> bad{0};
        const auto work = [&]() {
            for (uint64_t q = next++; q < host_pl.size(); q = next++) {
                const hc::SrCliquePl& P = pls[host_pl[q]];
                const uint32_t base_vertex = (uint32_t)key[clique_off[P.clique] + base_rank[P.clique]];
                uint32_t cls = 0;
                if (hc_host_sr_clique_filter(vert.data() + P.start, endpos.data() + P.start, P.n, num, base_vertex, 0, used.data() + P.start, &cls) != HC_OK)
                    bad = 1;
            }
        };
        const uint32_t n_threads = std::max<uint32_t>(1, std::min<uint64_t>(settings->n_threads, host_pl.size()));
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
        if (bad) return fail(HC_ERR_HIP, me + ": the host's filter refused a layout the device laid out");
        HC_HIP(hipMemcpyAsync(W.fused, used.data(), n_entries, hipMemcpyHostToDevice, s));
        HC_HIP(hipStreamSynchronize(s));  // (the host vector goes out of scope)
        ms_host_filter = ms_since(t0);
    }
    // 7. the packed outputs and the used members
    uint64_t n_used = 0;
    if (n_layouts) {
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hipMemsetAsync(B.uflag.p, 0, (n_members + 1) * 8, s));
        HC_HIP(hc::sr_clique_launch_compact(W, n_entries, s));
        HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.uflag, W.uoff, n_members + 1, s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(&n_used, W.uoff + n_members, 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(layouts, W.out_layouts, n_layouts * sizeof(hc_sr_layout), hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(members, W.out_members, n_members * sizeof(hc_sr_member), hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(member_vertex, W.out_vertex, n_members * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(member_used, W.out_used, n_members, hipMemcpyDeviceToHost, s));
        if (layout_filter) HC_HIP(hipMemcpyAsync(layout_filter, W.out_filter, n_layouts, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_layout += ms;
        if ((rc = hc::sr_consensus_room(c, settings, n_layouts, n_used))) return rc;
        HC_HIP(hc::sr_clique_launch_consensus_input(W, n_layouts, n_members, c->sr.layouts.as<hc_sr_layout>(), c->sr.members.as<hc_sr_member>(), s));
    }
    bool ret_late = false;
    const int rc_run =
        hc::sr_consensus_run(c, me.c_str(), n_layouts, n_used, settings, ret, status, out_off, cons_seq, cons_qual, cap, n_bytes, sr_stats, &ret_late);
    // (HC_ERR_ARG here is the room of cons_seq / cons_qual: everything but the bytes is filled, the subread infos included)
    if (rc_run != HC_OK && rc_run != HC_ERR_ARG) return rc_run;
    if (n_layouts && ret_late) {  // a layout failed late: its ret is the host's
        std::vector<hc::SrLayoutInfo> info(n_layouts);
        for (uint64_t l = 0; l < n_layouts; l++) info[l] = hc::SrLayoutInfo{ret[l], status[l], 0, 0};
        HC_HIP(hipMemcpyAsync(c->sr.info.p, info.data(), n_layouts * sizeof(hc::SrLayoutInfo), hipMemcpyHostToDevice, s));
        HC_HIP(hipStreamSynchronize(s));  // (the host vector goes out of scope)
    }
    // 8. calcSubreadInfo, in (clique, vertex) order
    if (N) {
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::sr_clique_launch_subreads(W, c->sr.info.as<hc::SrLayoutInfo>(), s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(subreads, W.sub, N * sizeof(hc_sr_subread_info), hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_layout += ms;
    }
    if (stats) {
        stats->n_filtered_layouts = n_filtered;
        stats->n_host_filters = n_host_class;
        stats->ms_layout = ms_layout;
        stats->ms_host_filter = ms_host_filter;
    }
    return rc_run;
}
