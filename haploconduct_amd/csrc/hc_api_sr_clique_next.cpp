// hc_api_sr_clique_next.cpp — hc_sr_clique_next (include/hcsr.h): what SRBuilder::cliquesToSuperreads does between the consensus of the
// cliques and find-next-overlaps, from the arrays hc_sr_clique_merge returned.  The arrays go up once; the kernels of
// hc_sr_clique_next_kernels.hip sort the cliques' vertices, build the cliques' entries, find every member's owner, mark, order and fill the
// tables; the vertices' half is hc_sr_merge_next's own kernels on the slots behind the cliques'; between them run
// hc_sr_merge_self_overlaps_kept's own run (sr_self_kept_run), hc_sr_set_next_reads' check kernel on the cliques' and then on the
// vertices' entries, and, from the gather on, hc_sr_set_next_reads' own tail (sr_next_store).  The slots and the tables live in the
// scratch of hc_sr_merge_next (hc_ctx::SrMergeNext), what only this call needs in hc_ctx::SrCliqueNext.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr_clique_next.h"
#include "hc_sr_next.h"

namespace {

int fail(int status, const std::string& what) { return hc::set_last_error(status, std::string("hc_sr_clique_next: ") + what); }

int bits_for(uint64_t n) {  // bits that hold every value below n
    int b = 1;
    while (b < 32 && (1ull << b) < n) b++;
    return b;
}

}  // namespace

extern "C" int hc_sr_clique_next(hc_ctx* c, const hc_sr_clique_next_input* in, const hc_sr_clique_next_settings* st, hc_sr_clique_next_output* out) {
    if (!c || !in || !st || !out) return fail(HC_ERR_ARG, "null argument");
    c->sr_mn.tables_drop();  // (hc_fno1_from_graph: cleared at the start, whatever this call returns, the tables an earlier one kept are no longer the iteration's)
    const uint64_t nc = in->n_cliques, nv = in->n_vertices, n_slots = nc + nv;
    if (nc >= (1ull << 31) || nv >= (1ull << 31) || n_slots >= (1ull << 31)) return fail(HC_ERR_ARG, "n_cliques + n_vertices is 2^31 or more");
    if ((nc && (!in->clique_off || !in->clique_status || !in->first_layout || !out->clique_kind || !out->clique_new_id || !out->overlap_pos ||
                !out->self_score || !out->srs || !out->sr_clique)) ||
        (nv && (!in->vertex_read || !in->vertex_fwd || !out->vertex_state || !out->nodes)) || !out->clique_off || !out->subread_off)
        return fail(HC_ERR_ARG, "null array");
    if (nc && in->clique_off[0] != 0) return fail(HC_ERR_ARG, "clique_off[0] is not 0");
    for (uint64_t i = 0; i < nc; i++)
        if (in->clique_off[i + 1] < in->clique_off[i]) return fail(HC_ERR_ARG, "clique_off descends");
    const uint64_t n_items = nc ? in->clique_off[nc] : 0, n_layouts = nc ? in->first_layout[nc] : 0, n_members = in->n_members;
    if (n_items >= (1ull << 31)) return fail(HC_ERR_ARG, "2^31 clique entries or more");
    if (n_items && (!in->clique_nodes || !in->subreads || !out->clique_nodes || !out->subreads)) return fail(HC_ERR_ARG, "null array");
    if (n_layouts > 2 * nc || (n_layouts && (!in->layouts || !in->status || !in->out_off)) || (n_members && !in->member_vertex) || n_members > 2 * n_items)
        return fail(HC_ERR_ARG, "first_layout[n_cliques] exceeds 2 n_cliques, n_members exceeds 2 N, or the layouts are missing");
    if (!(st->self.min_qual == st->self.min_qual)) return fail(HC_ERR_ARG, "self.min_qual is NaN");
    hc_ctx::SrNext& N = c->srn;
    hc_ctx::Sr& K = c->sr;
    if (!N.keep) return fail(HC_ERR_STATE, "hc_sr_keep_device is off");
    if (!c->have_reads || !N.raw_valid) return fail(HC_ERR_STATE, "no store whose raw arrays were kept (hc_sr_keep_device, then hc_set_reads)");
    if (!K.kept_valid) return fail(HC_ERR_STATE, "no kept consensus bytes (hc_sr_consensus, hc_sr_clique_merge or hc_sr_kept_load first)");
    out->n_srs = out->n_singles = out->n_trivials = out->n_paired = out->n_self_merged = out->new_read_count = 0;
    out->ms_device = out->ms_copy = 0;
    memset(&out->counts, 0, sizeof out->counts);
    memset(&out->self_stats, 0, sizeof out->self_stats);
    out->clique_off[0] = out->subread_off[0] = 0;
    if (n_slots == 0) {
        N.prev_traded = false;  // (hc_sr_fastq_write_text: the store this call read is the one in place)
        return HC_SR_NEXT_EMPTY;
    }
    // the host's pass: the vertex range tests and the owners of the first layouts' members
    const hc::cn::In H{in->clique_off, in->clique_nodes, in->clique_status, in->first_layout, in->layouts, in->member_vertex, in->status, in->out_off,
                       in->subreads, nc, n_items, n_layouts, n_members, nv};
    std::vector<uint8_t> bad;
    std::vector<hc::cn::Owner> own;
    if (!hc::cn::host_plan(H, bad, own)) return fail(HC_ERR_ARG, "the cliques' first layouts do not name ascending member ranges");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    hc_ctx::SrMergeNext& W = c->sr_mn;
    hc_ctx::SrCliqueNext& Q = c->sr_cn;
    const uint32_t n_reads = (uint32_t)(N.h_first.size() - 1);
    const uint64_t n_it = 2 * n_members;  // index entries at most
    const size_t scan_bytes = std::max(hc::prims::scan_temp_bytes(n_slots + 1, sizeof(uint64_t)), hc::prims::scan_temp_bytes(n_members + 1, sizeof(uint64_t)));
    const size_t temp_bytes = std::max({scan_bytes, hc::prims::sort_temp_bytes(n_items ? n_items : 1, sizeof(uint64_t), 0),
                                        hc::prims::sort_temp_bytes(n_it ? n_it : 1, sizeof(uint64_t), sizeof(uint32_t))});
    int rc;
    auto room = [&](hc_scratch& k, size_t bytes) { return k.ensure(bytes ? bytes : 16); };
    if ((rc = room(Q.off, (nc + 1) * 8)) || (rc = room(Q.nodes, n_items * 4)) || (rc = room(Q.cstatus, nc * 4)) || (rc = room(Q.first_layout, (nc + 1) * 8)) ||
        (rc = room(Q.layouts, n_layouts * sizeof(hc_sr_layout))) || (rc = room(Q.mvertex, n_members * 4)) || (rc = room(Q.lay_status, n_layouts * 4)) ||
        (rc = room(Q.out_off, (n_layouts + 1) * 8)) || (rc = room(Q.sub, n_items * sizeof(hc_sr_subread_info))) || (rc = room(Q.v_read, nv * 4)) ||
        (rc = room(Q.v_fwd, nv)) || (rc = room(Q.bad, nc)) || (rc = room(Q.own, own.size() * sizeof(hc::cn::Owner))) || (rc = room(Q.key_in, n_items * 8)) ||
        (rc = room(Q.key, n_items * 8)) || (rc = room(Q.m_item, n_members * 4)) || (rc = room(Q.m_owner, n_members * 4)) ||
        (rc = room(Q.m_cnt, (n_members + 1) * 8)) || (rc = room(Q.m_off, (n_members + 1) * 8)) || (rc = room(Q.sr_of, nc * 4)) ||
        (rc = room(Q.sub_cnt, (nc + 1) * 8)) || (rc = room(Q.pre_cnt, (nc + 1) * 8)) || (rc = room(Q.pre_off, (nc + 1) * 8)) ||
        (rc = room(Q.it_key_in, n_it * 8)) || (rc = room(Q.it_key, n_it * 8)) || (rc = room(Q.it_val_in, n_it * 4)) || (rc = room(Q.it_val, n_it * 4)) ||
        (rc = room(Q.temp, temp_bytes)) ||
        // the slots and the tables: hc_sr_merge_next's blocks
        (rc = room(W.entries, n_slots * sizeof(hc_sr_next_entry))) || (rc = room(W.status, n_slots * 4)) || (rc = room(W.cnt, (n_slots + 1) * 8)) ||
        (rc = room(W.bytes, (n_slots + 1) * 8)) || (rc = room(W.key, (n_slots + 1) * 8)) || (rc = room(W.rank, (n_slots + 1) * 8)) ||
        (rc = room(W.overlap_pos, nc * 4)) || (rc = room(W.visited, nv)) || (rc = room(W.t_kind, nc * 4)) || (rc = room(W.t_id, nc * 4)) ||
        (rc = room(W.t_v_state, nv * 4)) || (rc = room(W.t_nodes, nv * sizeof(hc_fno_read))) || (rc = room(W.t_srs, nc * sizeof(hc_fno_read))) ||
        (rc = room(W.t_sr_pair, nc * 4)) || (rc = room(W.t_clique_cnt, (nc + 1) * 8)) || (rc = room(W.t_clique_off, (nc + 1) * 8)) ||
        (rc = room(W.t_clique_nodes, n_it * 8)) || (rc = room(W.t_sub_off, (nc + 1) * 8)) || (rc = room(W.t_sub, n_items * sizeof(hc_fno_subread))) ||
        // the entries in their final order and what the gather's sums need: hc_sr_set_next_reads' own blocks
        (rc = N.entries.ensure(n_slots * sizeof(hc_sr_next_entry))) || (rc = N.status.ensure(n_slots * 4)) || (rc = N.cnt.ensure((n_slots + 1) * 8)) ||
        (rc = N.bytes.ensure((n_slots + 1) * 8)) || (rc = N.cnt_off.ensure((n_slots + 1) * 8)) || (rc = N.byte_off.ensure((n_slots + 1) * 8)) ||
        (rc = N.temp.ensure(scan_bytes ? scan_bytes : 16)) || (rc = N.extra_seq.ensure(1)) || (rc = N.extra_qual.ensure(1)))
        return rc;
    const auto t_up = std::chrono::steady_clock::now();
    auto up = [&](hc_scratch& k, const void* p, size_t bytes) { return bytes ? hipMemcpyAsync(k.p, p, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    const uint64_t zero_off[1] = {0};
    HC_HIP(up(Q.off, nc ? in->clique_off : zero_off, (nc + 1) * 8));
    HC_HIP(up(Q.nodes, in->clique_nodes, n_items * 4));
    HC_HIP(up(Q.cstatus, in->clique_status, nc * 4));
    HC_HIP(up(Q.first_layout, in->first_layout, nc ? (nc + 1) * 8 : 0));
    HC_HIP(up(Q.layouts, in->layouts, n_layouts * sizeof(hc_sr_layout)));
    HC_HIP(up(Q.mvertex, in->member_vertex, n_members * 4));
    HC_HIP(up(Q.lay_status, in->status, n_layouts * 4));
    HC_HIP(up(Q.out_off, in->out_off, n_layouts ? (n_layouts + 1) * 8 : 0));
    HC_HIP(up(Q.sub, in->subreads, n_items * sizeof(hc_sr_subread_info)));
    HC_HIP(up(Q.v_read, in->vertex_read, nv * 4));
    HC_HIP(up(Q.v_fwd, in->vertex_fwd, nv));
    HC_HIP(up(Q.bad, bad.data(), nc));
    HC_HIP(up(Q.own, own.data(), own.size() * sizeof(hc::cn::Owner)));
    HC_HIP(hipStreamSynchronize(s));
    double ms_copy = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    const hc::cn::In D{Q.off.as<uint64_t>(), Q.nodes.as<uint32_t>(), Q.cstatus.as<uint32_t>(), Q.first_layout.as<uint64_t>(), Q.layouts.as<hc_sr_layout>(),
                       Q.mvertex.as<uint32_t>(), Q.lay_status.as<uint32_t>(), Q.out_off.as<uint64_t>(), Q.sub.as<hc_sr_subread_info>(), nc, n_items,
                       n_layouts, n_members, nv};
    const hc::cn::Work X{Q.bad.as<uint8_t>(), Q.own.as<hc::cn::Owner>(), own.size(), Q.key_in.as<uint64_t>(), Q.key.as<uint64_t>(), Q.m_item.as<uint32_t>(),
                         Q.m_owner.as<uint32_t>(), Q.m_cnt.as<uint64_t>(), Q.m_off.as<uint64_t>(), Q.sr_of.as<uint32_t>(), Q.sub_cnt.as<uint64_t>(),
                         Q.pre_cnt.as<uint64_t>(), Q.pre_off.as<uint64_t>(), Q.it_key_in.as<uint64_t>(), Q.it_key.as<uint64_t>(), Q.it_val_in.as<uint32_t>(),
                         Q.it_val.as<uint32_t>()};
    // the slots: [0, n_cliques) the cliques, then the vertices.  SV: the vertices' slots as hc_sr_merge_next's kernels see a call of no pairs.
    const hc::mn::Slots S{W.entries.as<hc_sr_next_entry>(), W.status.as<uint32_t>(), W.cnt.as<uint64_t>(), W.bytes.as<uint64_t>(), W.key.as<uint64_t>(),
                          W.rank.as<uint64_t>(), W.overlap_pos.as<int32_t>(), nullptr, W.visited.as<uint8_t>()};
    const hc::mn::Slots SV{S.entries + nc, S.status + nc, S.cnt + nc, S.bytes + nc, S.key + nc, S.rank + nc, nullptr, nullptr, S.visited};
    const hc::mn::In DV{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Q.v_read.as<uint32_t>(), Q.v_fwd.as<uint8_t>(), nullptr,
                        nullptr, 0, 0, 0, nv, n_reads};
    const hc::mn::Tables T{W.t_kind.as<uint32_t>(), W.t_id.as<int32_t>(), W.t_v_state.as<uint32_t>(), W.t_nodes.as<hc_fno_read>(),
                           W.t_srs.as<hc_fno_read>(), W.t_sr_pair.as<uint32_t>(), W.t_clique_cnt.as<uint64_t>(), W.t_clique_off.as<uint64_t>(),
                           W.t_clique_nodes.as<uint64_t>(), W.t_sub_off.as<uint64_t>(), W.t_sub.as<hc_fno_subread>(), nullptr};
    float ms = 0;
    double ms_device = 0;
    // 1. the cliques' vertices in order, the members' owners, the cliques' entries
    HC_HIP(hipEventRecord(c->ev0, s));
    if (n_items) {
        HC_HIP(hc::cn::launch_items(D, X, s));
        HC_HIP(hc::prims::sort_keys(Q.temp.p, Q.temp.cap, X.key_in, X.key, n_items, 0, 32 + bits_for(nc), s));
    }
    HC_HIP(hc::cn::launch_members(D, X, s));
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, X.m_cnt, X.m_off, n_members + 1, s));
    if (nc) HC_HIP(hc::cn::launch_cliques(D, X, S, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));  // (read now: the self-overlap run records the context's events itself)
    ms_device += ms;
    for (uint64_t i = 0; i < nc; i++) {
        out->overlap_pos[i] = -1;
        out->self_score[i] = 0;
    }
    //    the self-overlap test of the paired ones with two mates (:983-985) on a pair list built from out_off
    std::vector<hc::mn::Rewrite> rw;  // (outlives its copy: the next wait on the stream is behind the rank sum)
    if (nc && !st->no_self_overlap) {
        std::vector<uint64_t> cand;
        std::vector<hc_sr_pair> self_pairs;
        for (uint64_t i = 0; i < nc; i++) {
            hc_sr_next_entry e;
            hc::cn::clique_entry(H, i, bad[i] != 0, e);
            if (!hc::mn::self_candidate(e)) continue;
            cand.push_back(i);
            self_pairs.push_back(hc_sr_pair{e.off1, e.off2, e.len1, e.len2});
        }
        if (!cand.empty()) {
            const uint64_t k = cand.size();
            std::vector<int32_t> pos(k);
            std::vector<double> score(k);
            std::vector<uint32_t> sst(k);
            std::vector<uint64_t> off(k + 1);
            uint64_t n_out = 0;
            if ((rc = hc::sr_self_kept_run(c, "hc_sr_clique_next: ", self_pairs.data(), k, &st->self, pos.data(), score.data(), sst.data(), off.data(), &n_out,
                                           &out->self_stats)))
                return rc;
            for (uint64_t a = 0; a < k; a++) {
                if (sst[a] != HC_SR_SELF_MERGED) continue;
                out->overlap_pos[cand[a]] = pos[a];
                out->self_score[cand[a]] = score[a];
                rw.push_back(hc::mn::Rewrite{off[a], (uint32_t)cand[a], (uint32_t)(off[a + 1] - off[a]), pos[a], 0});
            }
            out->n_self_merged = rw.size();
            if (!rw.empty()) {
                if ((rc = room(W.rewrite, rw.size() * sizeof(hc::mn::Rewrite)))) return rc;
                HC_HIP(hipMemcpyAsync(W.rewrite.p, rw.data(), rw.size() * sizeof(hc::mn::Rewrite), hipMemcpyHostToDevice, s));
                HC_HIP(hc::mn::launch_rewrite(W.rewrite.as<hc::mn::Rewrite>(), rw.size(), nc, S, s));
            }
        }
    }
    // 2. - 4. the tests, the marks, the trivials, the ranks
    const hc::SrNextSources src{K.kept_bytes, 0, N.off.as<uint64_t>(), N.first.as<uint32_t>(), n_reads};
    const hc::SrNextBytes B{{K.seq.as<uint8_t>(), N.extra_seq.as<uint8_t>(), N.bases.as<uint8_t>()},
                            {K.qual.as<uint8_t>(), N.extra_qual.as<uint8_t>(), N.quals.as<uint8_t>()}};
    HC_HIP(hipEventRecord(c->ev0, s));
    if (nv) HC_HIP(hipMemsetAsync(W.visited.p, 0, nv, s));
    if (nc) {
        HC_HIP(hc::sr_next_launch_check(S.entries, nc, src, B, st->keep_singletons, S.status, S.cnt, S.bytes, s));
        if (n_members) HC_HIP(hc::cn::launch_mark(D, X, S, s));
        HC_HIP(hc::cn::launch_keys(D, S, s));
    }
    if (nv) {
        HC_HIP(hc::mn::launch_vertices(DV, SV, src, s));
        HC_HIP(hc::sr_next_launch_check(SV.entries, nv, src, B, st->keep_singletons, SV.status, SV.cnt, SV.bytes, s));
        HC_HIP(hc::mn::launch_vertex_finish(DV, SV, 0, 0, T, s));
    } else {
        HC_HIP(hipMemsetAsync(S.key + n_slots, 0, 8, s));
    }
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, S.key, S.rank, n_slots + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t r[2] = {0, 0};  // singles | paired << 32 over the cliques; that + trivials over all
    HC_HIP(hipMemcpyAsync(&r[0], S.rank + nc, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&r[1], S.rank + n_slots, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    hc::mn::Totals tot;
    tot.n_singles = (uint32_t)r[0];
    tot.n_paired = (uint32_t)(r[0] >> 32);
    tot.n_trivials = (uint32_t)r[1] - tot.n_singles;
    tot.n_tips = 0;
    const uint64_t n_srs = (uint64_t)tot.n_singles + tot.n_paired, n_kept = n_srs + tot.n_trivials;
    // the entries in final order, the gather's sums, the sizes of the rows, of the subread lists and of the self-merged cliques' entries
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::cn::launch_order(D, X, S, tot, N.entries.as<hc_sr_next_entry>(), N.status.as<uint32_t>(), N.cnt.as<uint64_t>(), N.bytes.as<uint64_t>(), T, s));
    HC_HIP(hc::mn::launch_order(DV, SV, tot, src, N.entries.as<hc_sr_next_entry>(), N.status.as<uint32_t>(), N.cnt.as<uint64_t>(), N.bytes.as<uint64_t>(), T, s));
    HC_HIP(hc::prims::exclusive_sum(N.temp.p, N.temp.cap, N.cnt.as<uint64_t>(), N.cnt_off.as<uint64_t>(), n_kept + 1, s));
    HC_HIP(hc::prims::exclusive_sum(N.temp.p, N.temp.cap, N.bytes.as<uint64_t>(), N.byte_off.as<uint64_t>(), n_kept + 1, s));
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, T.clique_cnt, T.clique_off, n_srs + 1, s));
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, X.sub_cnt, T.subread_off, n_srs + 1, s));
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, X.pre_cnt, X.pre_off, n_srs + 1, s));
    if (n_srs && n_members) HC_HIP(hc::cn::launch_member_rows(D, X, S, T, s));
    if (n_srs && n_items) HC_HIP(hc::cn::launch_subreads(D, X, S, T, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    auto down = [&](void* dst, const void* p, size_t bytes) { return bytes ? hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
    uint64_t sums[4] = {0, 0, 0, 0};  // kept | sequences << 32, bytes, index entries, row entries
    HC_HIP(down(&sums[0], N.cnt_off.as<uint64_t>() + n_kept, 8));
    HC_HIP(down(&sums[1], N.byte_off.as<uint64_t>() + n_kept, 8));
    HC_HIP(down(&sums[2], X.pre_off + n_srs, 8));
    HC_HIP(down(&sums[3], T.clique_off + n_srs, 8));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    const uint64_t n_entries = sums[2], n_rows = sums[3];
    if (n_entries > n_it || n_rows > n_it) return fail(HC_ERR_STATE, "the rows left their bound");
    // 5. the self-merged cliques' rows: one stable sort of all their index entries by (super-read, index)
    HC_HIP(hipEventRecord(c->ev0, s));
    if (n_entries) {
        HC_HIP(hc::prims::sort_pairs(Q.temp.p, Q.temp.cap, X.it_key_in, X.it_key, X.it_val_in, X.it_val, n_entries, 0, 32 + bits_for(n_srs), s));
        HC_HIP(hc::cn::launch_merged_rows(X, n_entries, T, s));
    }
    HC_HIP(hipEventRecord(c->ev1, s));
    const auto t_down = std::chrono::steady_clock::now();
    if (n_rows > 2 * n_items) return fail(HC_ERR_ARG, "the rows hold more than 2 N vertices: clique_nodes has no room for them");
    HC_HIP(down(out->clique_kind, T.pair_kind, nc * 4));
    HC_HIP(down(out->clique_new_id, T.pair_new_id, nc * 4));
    HC_HIP(down(out->vertex_state, T.vertex_state, nv * 4));
    HC_HIP(down(out->nodes, T.nodes, nv * sizeof(hc_fno_read)));
    HC_HIP(down(out->srs, T.srs, n_srs * sizeof(hc_fno_read)));
    HC_HIP(down(out->sr_clique, T.sr_pair, n_srs * 4));
    HC_HIP(down(out->clique_off, T.clique_off, (n_srs + 1) * 8));
    HC_HIP(down(out->subread_off, T.subread_off, (n_srs + 1) * 8));
    HC_HIP(down(out->clique_nodes, T.clique_nodes, n_rows * 8));
    HC_HIP(hipStreamSynchronize(s));
    const uint64_t n_sub = out->subread_off[n_srs];
    if (n_sub > n_items) return fail(HC_ERR_STATE, "the subread lists left their bound");
    HC_HIP(down(out->subreads, T.subreads, n_sub * sizeof(hc_fno_subread)));
    HC_HIP(hipStreamSynchronize(s));
    ms_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    out->n_srs = n_srs;
    out->n_singles = tot.n_singles;
    out->n_paired = tot.n_paired;
    out->n_trivials = tot.n_trivials;
    out->new_read_count = n_kept;
    hc_sr_next_counts cn;
    memset(&cn, 0, sizeof cn);
    for (uint64_t i = 0; i < nc; i++) {
        cn.n_dropped_empty += out->clique_kind[i] == HC_SR_MN_DROPPED_EMPTY;
        cn.n_dropped_n_rate += out->clique_kind[i] == HC_SR_MN_DROPPED_N_RATE;
        cn.n_bad += out->clique_kind[i] == HC_SR_MN_NONE;
    }
    for (uint64_t v = 0; v < nv; v++) {
        cn.n_dropped_short += out->vertex_state[v] == HC_SR_MN_V_SHORT;
        cn.n_dropped_n_rate += out->vertex_state[v] == HC_SR_MN_V_N_RATE;
        cn.n_bad += out->vertex_state[v] == HC_SR_MN_V_BAD;
    }
    cn.n_kept = n_kept;
    cn.n_seq = (uint32_t)(sums[0] >> 32);
    cn.n_bytes = sums[1];
    out->counts = cn;
    out->ms_device = ms_device;
    out->ms_copy = ms_copy;
    if ((uint32_t)sums[0] != n_kept) return fail(HC_ERR_STATE, "the ranks and the gather's count of survivors disagree");
    if (n_kept == 0) {  // the old store stays
        N.prev_traded = false;
        return HC_SR_NEXT_EMPTY;
    }
    // the store, by hc_sr_set_next_reads' own tail
    if ((rc = hc::sr_next_store(c, n_kept, 0, (uint32_t)n_kept, (uint32_t)cn.n_seq, cn.n_bytes, cn))) return rc;
    out->counts = cn;  // (counts.ms_device: the gather and the histograms; ms_device: this section's own kernels)
    W.tables_valid = true, W.tables_vertices = nv, W.tables_srs = n_srs, W.tables_new_read_count = n_kept;
    return HC_OK;
}
