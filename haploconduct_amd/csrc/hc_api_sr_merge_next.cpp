// hc_api_sr_merge_next.cpp — hc_sr_merge_next (include/hcsr.h): what SRBuilder::mergeAlongEdges does between the consensus of the picked
// edges and find-next-overlaps, from the arrays hc_sr_edge_merge returned.  The arrays go up once; the kernels of
// hc_sr_merge_next_kernels.hip build the pairs' entries, mark, build the trivials, order and fill the tables; between them run
// hc_sr_merge_self_overlaps_kept's own run (hc_api_sr.cpp: sr_self_kept_run), hc_sr_set_next_reads' check kernel on the pairs' and
// then on the vertices' entries, and, from the gather on, hc_sr_set_next_reads' own tail (hc_api_sr_next.cpp: sr_next_store).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr_merge_next.h"
#include "hc_sr_next.h"

namespace {

int fail(int status, const std::string& what) { return hc::set_last_error(status, std::string("hc_sr_merge_next: ") + what); }

}  // namespace

extern "C" int hc_sr_merge_next(hc_ctx* c, const hc_sr_merge_next_input* in, const hc_sr_merge_next_settings* st, hc_sr_merge_next_output* out) {
    if (!c || !in || !st || !out) return fail(HC_ERR_ARG, "null argument");
    c->sr_mn.tables_drop();  // (hc_fno1_from_graph: cleared at the start, whatever this call returns, the tables an earlier one kept are no longer the iteration's)
    const uint64_t np = in->n_pairs, nv = in->n_vertices, n_slots = np + nv;
    if (np >= (1ull << 31) || nv >= (1ull << 31) || n_slots >= (1ull << 31)) return fail(HC_ERR_ARG, "n_pairs + n_vertices is 2^31 or more");
    if ((np && (!in->pairs || !in->pair_status || !in->first_layout || !in->subreads || !out->pair_kind || !out->pair_new_id || !out->overlap_pos ||
                !out->self_score || !out->srs || !out->sr_pair || !out->clique_nodes || !out->subreads)) ||
        (nv && (!in->vertex_read || !in->vertex_fwd || !out->vertex_state || !out->nodes || !out->tips)) || !out->clique_off || !out->subread_off)
        return fail(HC_ERR_ARG, "null array");
    const uint64_t n_layouts = np ? in->first_layout[np] : 0, n_members = in->n_members;
    if (n_layouts > 2 * np || (n_layouts && (!in->layouts || !in->status || !in->out_off)) || (n_members && !in->members) || n_members > 6 * np)
        return fail(HC_ERR_ARG, "first_layout[n_pairs] exceeds 2 n_pairs, n_members exceeds 6 n_pairs, or the layouts are missing");
    if (!(st->self.min_qual == st->self.min_qual)) return fail(HC_ERR_ARG, "self.min_qual is NaN");
    hc_ctx::SrNext& N = c->srn;
    hc_ctx::Sr& K = c->sr;
    if (!N.keep) return fail(HC_ERR_STATE, "hc_sr_keep_device is off");
    if (!c->have_reads || !N.raw_valid) return fail(HC_ERR_STATE, "no store whose raw arrays were kept (hc_sr_keep_device, then hc_set_reads)");
    if (!K.kept_valid) return fail(HC_ERR_STATE, "no kept consensus bytes (hc_sr_consensus, hc_sr_edge_merge or hc_sr_kept_load first)");
    out->n_srs = out->n_singles = out->n_trivials = out->n_paired = out->n_tips = out->n_self_merged = out->new_read_count = 0;
    out->ms_device = out->ms_copy = 0;
    memset(&out->counts, 0, sizeof out->counts);
    memset(&out->self_stats, 0, sizeof out->self_stats);
    out->clique_off[0] = out->subread_off[0] = 0;
    if (n_slots == 0) {
        N.prev_traded = false;  // (hc_sr_fastq_write_text: the store this call read is the one in place)
        return HC_SR_NEXT_EMPTY;
    }
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    hc_ctx::SrMergeNext& W = c->sr_mn;
    const uint32_t n_reads = (uint32_t)(N.h_first.size() - 1);
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n_slots + 1, sizeof(uint64_t));
    int rc;
    auto room = [&](hc_scratch& k, size_t bytes) { return k.ensure(bytes ? bytes : 16); };
    if ((rc = room(W.pairs, np * 8)) || (rc = room(W.pair_status, np * 4)) || (rc = room(W.first_layout, (np + 1) * 8)) ||
        (rc = room(W.layouts, n_layouts * sizeof(hc_sr_layout))) || (rc = room(W.members, n_members * sizeof(hc_sr_member))) ||
        (rc = room(W.lay_status, n_layouts * 4)) || (rc = room(W.out_off, (n_layouts + 1) * 8)) || (rc = room(W.sub, np * 2 * sizeof(hc_sr_subread_info))) ||
        (rc = room(W.v_read, nv * 4)) || (rc = room(W.v_fwd, nv)) || (rc = room(W.incl, nv)) || (rc = room(W.tip_reads, n_reads)) ||
        (rc = room(W.entries, n_slots * sizeof(hc_sr_next_entry))) || (rc = room(W.status, n_slots * 4)) || (rc = room(W.cnt, (n_slots + 1) * 8)) ||
        (rc = room(W.bytes, (n_slots + 1) * 8)) || (rc = room(W.key, (n_slots + 1) * 8)) || (rc = room(W.rank, (n_slots + 1) * 8)) ||
        (rc = room(W.overlap_pos, np * 4)) || (rc = room(W.n_clique, np)) || (rc = room(W.visited, nv)) || (rc = room(W.t_kind, np * 4)) ||
        (rc = room(W.t_id, np * 4)) || (rc = room(W.t_v_state, nv * 4)) || (rc = room(W.t_nodes, nv * sizeof(hc_fno_read))) ||
        (rc = room(W.t_srs, np * sizeof(hc_fno_read))) || (rc = room(W.t_sr_pair, np * 4)) || (rc = room(W.t_clique_cnt, (np + 1) * 8)) ||
        (rc = room(W.t_clique_off, (np + 1) * 8)) || (rc = room(W.t_clique_nodes, np * 4 * 8)) || (rc = room(W.t_sub_off, (np + 1) * 8)) ||
        (rc = room(W.t_sub, np * 2 * sizeof(hc_fno_subread))) || (rc = room(W.t_tips, nv * 4)) || (rc = room(W.temp, scan_bytes)) ||
        // the entries in their final order and what the gather's sums need: hc_sr_set_next_reads' own blocks
        (rc = N.entries.ensure(n_slots * sizeof(hc_sr_next_entry))) || (rc = N.status.ensure(n_slots * 4)) || (rc = N.cnt.ensure((n_slots + 1) * 8)) ||
        (rc = N.bytes.ensure((n_slots + 1) * 8)) || (rc = N.cnt_off.ensure((n_slots + 1) * 8)) || (rc = N.byte_off.ensure((n_slots + 1) * 8)) ||
        (rc = N.temp.ensure(scan_bytes ? scan_bytes : 16)) || (rc = N.extra_seq.ensure(1)) || (rc = N.extra_qual.ensure(1)))
        return rc;
    const auto t_up = std::chrono::steady_clock::now();
    auto up = [&](hc_scratch& k, const void* p, size_t bytes) { return bytes ? hipMemcpyAsync(k.p, p, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    HC_HIP(up(W.pairs, in->pairs, np * 8));
    HC_HIP(up(W.pair_status, in->pair_status, np * 4));
    HC_HIP(up(W.first_layout, in->first_layout, np ? (np + 1) * 8 : 0));
    HC_HIP(up(W.layouts, in->layouts, n_layouts * sizeof(hc_sr_layout)));
    HC_HIP(up(W.members, in->members, n_members * sizeof(hc_sr_member)));
    HC_HIP(up(W.lay_status, in->status, n_layouts * 4));
    HC_HIP(up(W.out_off, in->out_off, n_layouts ? (n_layouts + 1) * 8 : 0));
    HC_HIP(up(W.sub, in->subreads, np * 2 * sizeof(hc_sr_subread_info)));
    HC_HIP(up(W.v_read, in->vertex_read, nv * 4));
    HC_HIP(up(W.v_fwd, in->vertex_fwd, nv));
    if (in->inclusions) HC_HIP(up(W.incl, in->inclusions, nv));
    if (in->tip_reads) HC_HIP(up(W.tip_reads, in->tip_reads, n_reads));
    HC_HIP(hipStreamSynchronize(s));
    double ms_copy = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    const hc::mn::In D{W.pairs.as<uint32_t>(), W.pair_status.as<uint32_t>(), W.first_layout.as<uint64_t>(), W.layouts.as<hc_sr_layout>(),
                       W.members.as<hc_sr_member>(), W.lay_status.as<uint32_t>(), W.out_off.as<uint64_t>(), W.sub.as<hc_sr_subread_info>(),
                       W.v_read.as<uint32_t>(), W.v_fwd.as<uint8_t>(), in->inclusions ? W.incl.as<uint8_t>() : nullptr,
                       in->tip_reads ? W.tip_reads.as<uint8_t>() : nullptr, np, n_layouts, n_members, nv, n_reads};
    const hc::mn::In H{in->pairs, in->pair_status, in->first_layout, in->layouts, in->members, in->status, in->out_off, in->subreads, in->vertex_read,
                       in->vertex_fwd, in->inclusions, in->tip_reads, np, n_layouts, n_members, nv, n_reads};
    const hc::mn::Slots S{W.entries.as<hc_sr_next_entry>(), W.status.as<uint32_t>(), W.cnt.as<uint64_t>(), W.bytes.as<uint64_t>(),
                          W.key.as<uint64_t>(), W.rank.as<uint64_t>(), W.overlap_pos.as<int32_t>(), W.n_clique.as<uint8_t>(),
                          W.visited.as<uint8_t>()};
    const hc::mn::Tables T{W.t_kind.as<uint32_t>(), W.t_id.as<int32_t>(), W.t_v_state.as<uint32_t>(), W.t_nodes.as<hc_fno_read>(),
                           W.t_srs.as<hc_fno_read>(), W.t_sr_pair.as<uint32_t>(), W.t_clique_cnt.as<uint64_t>(), W.t_clique_off.as<uint64_t>(),
                           W.t_clique_nodes.as<uint64_t>(), W.t_sub_off.as<uint64_t>(), W.t_sub.as<hc_fno_subread>(), W.t_tips.as<uint32_t>()};
    float ms = 0;
    double ms_device = 0;
    // 1. the pairs' entries; the self-overlap test of the paired ones with two mates (:983-985) on a pair list built from out_off
    if (np) HC_HIP(hc::mn::launch_pairs(D, S, s));
    for (uint64_t i = 0; i < np; i++) {
        out->overlap_pos[i] = -1;
        out->self_score[i] = 0;
    }
    if (np && !st->no_self_overlap) {
        std::vector<uint64_t> cand;
        std::vector<hc_sr_pair> self_pairs;
        for (uint64_t i = 0; i < np; i++) {
            hc_sr_next_entry e;
            uint32_t nc;
            hc::mn::pair_entry(H, i, e, nc);
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
            if ((rc = hc::sr_self_kept_run(c, "hc_sr_merge_next: ", self_pairs.data(), k, &st->self, pos.data(), score.data(), sst.data(), off.data(), &n_out,
                                           &out->self_stats)))
                return rc;
            std::vector<hc::mn::Rewrite> rw;
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
                HC_HIP(hc::mn::launch_rewrite(W.rewrite.as<hc::mn::Rewrite>(), rw.size(), np, S, s));
                HC_HIP(hipStreamSynchronize(s));  // (rw leaves scope)
            }
        }
    }
    // 2. - 4. the tests, the marks, the trivials, the ranks
    const hc::SrNextSources src{K.kept_bytes, 0, N.off.as<uint64_t>(), N.first.as<uint32_t>(), n_reads};
    const hc::SrNextBytes B{{K.seq.as<uint8_t>(), N.extra_seq.as<uint8_t>(), N.bases.as<uint8_t>()},
                            {K.qual.as<uint8_t>(), N.extra_qual.as<uint8_t>(), N.quals.as<uint8_t>()}};
    HC_HIP(hipEventRecord(c->ev0, s));
    if (nv) HC_HIP(hipMemsetAsync(W.visited.p, 0, nv, s));
    if (np) {
        HC_HIP(hc::sr_next_launch_check(S.entries, np, src, B, st->keep_singletons, S.status, S.cnt, S.bytes, s));
        HC_HIP(hc::mn::launch_mark(D, S, s));
    }
    if (nv) {
        HC_HIP(hc::mn::launch_vertices(D, S, src, s));
        HC_HIP(hc::sr_next_launch_check(S.entries + np, nv, src, B, st->keep_singletons, S.status + np, S.cnt + np, S.bytes + np, s));
        HC_HIP(hc::mn::launch_vertex_finish(D, S, st->ignore_inclusions, st->store_tips_separately, T, s));
    } else {
        HC_HIP(hipMemsetAsync(S.key + n_slots, 0, 8, s));
    }
    HC_HIP(hc::prims::exclusive_sum(W.temp.p, W.temp.cap, S.key, S.rank, n_slots + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t r[2] = {0, 0};  // singles | paired << 32 over the pairs; that + trivials | tips << 32 over all
    HC_HIP(hipMemcpyAsync(&r[0], S.rank + np, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&r[1], S.rank + n_slots, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    hc::mn::Totals tot;
    tot.n_singles = (uint32_t)r[0];
    tot.n_paired = (uint32_t)(r[0] >> 32);
    tot.n_trivials = (uint32_t)r[1] - tot.n_singles;
    tot.n_tips = (uint32_t)(r[1] >> 32) - tot.n_paired;
    const uint64_t n_srs = (uint64_t)tot.n_singles + tot.n_paired, n_kept = n_srs + tot.n_trivials;
    // the entries in final order, the gather's sums, the tables
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::mn::launch_order(D, S, tot, src, N.entries.as<hc_sr_next_entry>(), N.status.as<uint32_t>(), N.cnt.as<uint64_t>(), N.bytes.as<uint64_t>(), T, s));
    HC_HIP(hc::prims::exclusive_sum(N.temp.p, N.temp.cap, N.cnt.as<uint64_t>(), N.cnt_off.as<uint64_t>(), n_kept + 1, s));
    HC_HIP(hc::prims::exclusive_sum(N.temp.p, N.temp.cap, N.bytes.as<uint64_t>(), N.byte_off.as<uint64_t>(), n_kept + 1, s));
    HC_HIP(hc::prims::exclusive_sum(W.temp.p, W.temp.cap, T.clique_cnt, T.clique_off, n_srs + 1, s));
    if (n_srs) HC_HIP(hc::mn::launch_tables(D, S, n_srs, T, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    const auto t_down = std::chrono::steady_clock::now();
    uint64_t sums[2] = {0, 0};  // kept | sequences << 32, bytes
    auto down = [&](void* dst, const void* p, size_t bytes) { return bytes ? hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
    HC_HIP(down(&sums[0], N.cnt_off.as<uint64_t>() + n_kept, 8));
    HC_HIP(down(&sums[1], N.byte_off.as<uint64_t>() + n_kept, 8));
    HC_HIP(down(out->pair_kind, T.pair_kind, np * 4));
    HC_HIP(down(out->pair_new_id, T.pair_new_id, np * 4));
    HC_HIP(down(out->vertex_state, T.vertex_state, nv * 4));
    HC_HIP(down(out->nodes, T.nodes, nv * sizeof(hc_fno_read)));
    HC_HIP(down(out->srs, T.srs, n_srs * sizeof(hc_fno_read)));
    HC_HIP(down(out->sr_pair, T.sr_pair, n_srs * 4));
    HC_HIP(down(out->clique_off, T.clique_off, (n_srs + 1) * 8));
    HC_HIP(down(out->subread_off, T.subread_off, n_srs ? (n_srs + 1) * 8 : 0));
    HC_HIP(down(out->subreads, T.subreads, n_srs * 2 * sizeof(hc_fno_subread)));
    HC_HIP(down(out->tips, T.tips, (size_t)tot.n_tips * 4));
    HC_HIP(hipStreamSynchronize(s));
    const uint64_t n_clique = out->clique_off[n_srs];
    if (n_clique > 4 * np) return fail(HC_ERR_STATE, "the cliques hold more than four vertices a super-read");
    HC_HIP(down(out->clique_nodes, T.clique_nodes, n_clique * 8));
    HC_HIP(hipStreamSynchronize(s));
    ms_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    out->n_srs = n_srs;
    out->n_singles = tot.n_singles;
    out->n_paired = tot.n_paired;
    out->n_trivials = tot.n_trivials;
    out->n_tips = tot.n_tips;
    out->new_read_count = n_kept;
    hc_sr_next_counts cn;
    memset(&cn, 0, sizeof cn);
    for (uint64_t i = 0; i < np; i++) {
        cn.n_dropped_empty += out->pair_kind[i] == HC_SR_MN_DROPPED_EMPTY;
        cn.n_dropped_n_rate += out->pair_kind[i] == HC_SR_MN_DROPPED_N_RATE;
        cn.n_bad += out->pair_kind[i] == HC_SR_MN_NONE;
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
    // 5. the store, by hc_sr_set_next_reads' own tail
    if ((rc = hc::sr_next_store(c, n_kept, 0, (uint32_t)n_kept, (uint32_t)cn.n_seq, cn.n_bytes, cn))) return rc;
    out->counts = cn;  // (counts.ms_device: the gather and the histograms; ms_device: this section's own kernels)
    W.tables_valid = true, W.tables_vertices = nv, W.tables_srs = n_srs, W.tables_new_read_count = n_kept;
    return HC_OK;
}
