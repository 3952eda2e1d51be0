// SrCliqueNext.cpp — hc_host_sr_clique_next and hc_host_sr_clique_select (include/hcsr.h).  The first is the host mirror of
// hc_sr_clique_next: it walks the loops of SRBuilder::process_cliques (reference src/SRBuilder.cpp:978-1003), merge_self_overlap's
// re-indexing (:911-935) and cliquesToSuperreads (:1122-1233) as they are written, one thread, over the mirrors of the steps in between:
// hc_host_sr_merge_self_overlaps for merge_self_overlap and hc_host_sr_next_reads for test_N_rate, get_len, the numbering and the bytes.
// The expressions it shares with the device are those of hc_sr_clique_next.h and hc_sr_merge_next.h.  The second is the gate of
// :1056-1084 in front of process_cliques.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/hcsr.h"
#include "../hc_ctx.h"
#include "../hc_sr_clique_next.h"

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

}  // namespace

extern "C" int hc_host_sr_clique_next(const hc_settings* ec_settings, const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off,
                                      const uint32_t* read_first_seq, uint32_t n_reads, const uint8_t* cons_seq, const uint8_t* cons_qual,
                                      uint64_t n_cons, const hc_sr_clique_next_input* in, const hc_sr_clique_next_settings* st,
                                      hc_sr_clique_next_output* out, uint8_t* out_bases, uint8_t* out_quals, uint64_t cap, uint64_t* n_bytes,
                                      uint64_t* out_seq_off, uint32_t* out_read_first_seq) {
    const char* me = "hc_host_sr_clique_next";
    if (!ec_settings || !in || !st || !out || !n_bytes || !out_seq_off || !out_read_first_seq || (n_cons && (!cons_seq || !cons_qual)) ||
        (n_reads && (!seq_off || !read_first_seq)))
        return fail(me, HC_ERR_ARG, "null argument");
    const uint64_t nc = in->n_cliques, nv = in->n_vertices, n_slots = nc + nv;
    if (n_slots >= (1ull << 31)) return fail(me, HC_ERR_ARG, "n_cliques + n_vertices is 2^31 or more");
    if ((nc && (!in->clique_off || !in->clique_status || !in->first_layout || !out->clique_kind || !out->clique_new_id || !out->overlap_pos ||
                !out->self_score || !out->srs || !out->sr_clique)) ||
        (nv && (!in->vertex_read || !in->vertex_fwd || !out->vertex_state || !out->nodes)) || !out->clique_off || !out->subread_off)
        return fail(me, HC_ERR_ARG, "null array");
    if (nc && in->clique_off[0] != 0) return fail(me, HC_ERR_ARG, "clique_off[0] is not 0");
    for (uint64_t i = 0; i < nc; i++)
        if (in->clique_off[i + 1] < in->clique_off[i]) return fail(me, HC_ERR_ARG, "clique_off descends");
    const uint64_t n_items = nc ? in->clique_off[nc] : 0, n_layouts = nc ? in->first_layout[nc] : 0, n_members = in->n_members;
    if (n_items >= (1ull << 31)) return fail(me, HC_ERR_ARG, "2^31 clique entries or more");
    if (n_items && (!in->clique_nodes || !in->subreads || !out->clique_nodes || !out->subreads)) return fail(me, HC_ERR_ARG, "null array");
    if (n_layouts > 2 * nc || (n_layouts && (!in->layouts || !in->status || !in->out_off)) || (n_members && !in->member_vertex) || n_members > 2 * n_items)
        return fail(me, HC_ERR_ARG, "first_layout[n_cliques] exceeds 2 n_cliques, n_members exceeds 2 N, or the layouts are missing");
    const hc::cn::In I{in->clique_off, in->clique_nodes, in->clique_status, in->first_layout, in->layouts, in->member_vertex, in->status, in->out_off,
                       in->subreads, nc, n_items, n_layouts, n_members, nv};
    std::vector<uint8_t> bad;
    std::vector<hc::cn::Owner> own;
    if (!hc::cn::host_plan(I, bad, own)) return fail(me, HC_ERR_ARG, "the cliques' first layouts do not name ascending member ranges");
    out->n_srs = out->n_singles = out->n_trivials = out->n_paired = out->n_self_merged = out->new_read_count = 0;
    out->ms_device = out->ms_copy = 0;
    memset(&out->counts, 0, sizeof out->counts);
    memset(&out->self_stats, 0, sizeof out->self_stats);
    out->clique_off[0] = out->subread_off[0] = 0;
    *n_bytes = 0;

    // process_cliques, :978-1003: constructSuperread's result per clique, then merge_self_overlap for a paired one with two mates
    std::vector<hc_sr_next_entry> pe(nc);
    std::vector<uint64_t> cand;
    std::vector<hc_sr_pair> self_pairs;
    for (uint64_t i = 0; i < nc; i++) {
        hc::cn::clique_entry(I, i, bad[i] != 0, pe[i]);
        out->overlap_pos[i] = -1;
        out->self_score[i] = 0;
        if (st->no_self_overlap || !hc::mn::self_candidate(pe[i])) continue;  // :983
        cand.push_back(i);
        self_pairs.push_back(hc_sr_pair{pe[i].off1, pe[i].off2, pe[i].len1, pe[i].len2});
    }
    std::vector<uint8_t> kept_seq(cons_seq, cons_seq + n_cons), kept_qual(cons_qual, cons_qual + n_cons);
    if (!cand.empty()) {
        const uint64_t k = cand.size();
        std::vector<int32_t> pos(k);
        std::vector<double> score(k);
        std::vector<uint32_t> sst(k);
        std::vector<uint64_t> off(k + 1);
        uint64_t n_out = 0;
        int rc = hc_host_sr_merge_self_overlaps(ec_settings, cons_seq, cons_qual, n_cons, self_pairs.data(), k, &st->self, pos.data(), score.data(),
                                                sst.data(), off.data(), nullptr, nullptr, 0, &n_out, &out->self_stats);  // count ...
        if (rc != HC_OK && !(rc == HC_ERR_ARG && n_out)) return rc;
        if (n_out) {
            kept_seq.resize(n_cons + n_out);
            kept_qual.resize(n_cons + n_out);
            rc = hc_host_sr_merge_self_overlaps(ec_settings, cons_seq, cons_qual, n_cons, self_pairs.data(), k, &st->self, pos.data(), score.data(),
                                                sst.data(), off.data(), kept_seq.data() + n_cons, kept_qual.data() + n_cons, n_out, &n_out,
                                                &out->self_stats);  // ... then fetch, behind the kept bytes as the kept form appends
            if (rc != HC_OK) return rc;
        }
        for (uint64_t a = 0; a < k; a++) {
            if (sst[a] != HC_SR_SELF_MERGED) continue;  // return superread, :954
            const uint64_t i = cand[a];
            out->overlap_pos[i] = pos[a];
            out->self_score[i] = score[a];
            pe[i] = hc_sr_next_entry{n_cons + off[a], 0, (uint32_t)(off[a + 1] - off[a]), 0, 0, HC_SR_NEXT_SINGLE, HC_SR_SRC_CONSENSUS, HC_SR_SRC_CONSENSUS, 0};
            out->n_self_merged++;
        }
    }
    // the tests of :983, :986, :999 on what is left: hc_host_sr_next_reads' statuses (no bytes asked for)
    hc_sr_next_settings ns{st->keep_singletons, 0};
    std::vector<int32_t> tmp_id(n_slots ? n_slots : 1);
    std::vector<uint32_t> pst(nc ? nc : 1), vst(nv ? nv : 1);
    std::vector<uint64_t> tmp_off(2 * n_slots + 1);
    std::vector<uint32_t> tmp_first(n_slots + 1);
    uint64_t nb = 0;
    const uint64_t n_kept_bytes = kept_seq.size();
    auto statuses = [&](const std::vector<hc_sr_next_entry>& e, uint64_t n, uint32_t* status) -> int {
        if (!n) return HC_OK;
        const int rc = hc_host_sr_next_reads(bases, quals, seq_off, read_first_seq, n_reads, kept_seq.data(), kept_qual.data(), n_kept_bytes, e.data(), n,
                                             nullptr, nullptr, 0, &ns, tmp_id.data(), status, nullptr, nullptr, nullptr, 0, &nb, tmp_off.data(),
                                             tmp_first.data());
        return (rc == HC_OK || rc == HC_SR_NEXT_EMPTY || (rc == HC_ERR_ARG && nb)) ? HC_OK : rc;
    };
    int rc = statuses(pe, nc, pst.data());
    if (rc) return rc;
    // :1122-1136: get_sorted_clique(0) / (1) of single_SR_vec's and paired_SR_vec's reads — sorted_vertices1, the first layout's full list
    std::vector<uint8_t> visited(nv ? nv : 1, 0);
    for (uint64_t i = 0; i < nc; i++) {
        out->clique_kind[i] = hc::mn::pair_kind(pe[i].kind, pst[i], out->overlap_pos[i] >= 0);
        if (pst[i] != HC_SR_NEXT_KEPT) continue;
        const hc_sr_layout L = in->layouts[in->first_layout[i]];
        for (uint64_t m = L.first_member; m < L.first_member + L.n_members; m++) visited[in->member_vertex[m]] = 1;
    }
    // :1145-1222
    std::vector<hc_sr_next_entry> ve(nv);
    for (uint64_t v = 0; v < nv; v++) {
        const uint32_t read = in->vertex_read[v];
        const uint32_t nm = read < n_reads ? read_first_seq[read + 1] - read_first_seq[read] : 0;
        ve[v] = hc_sr_next_entry{0, 0, 0, 0, read, hc::mn::kNoEntry, 0, 0, (uint8_t)(in->vertex_fwd[v] ? 0 : 1)};
        if (!visited[v]) ve[v].kind = nm == 2 ? HC_SR_NEXT_TRIVIAL_PAIRED : HC_SR_NEXT_TRIVIAL;
    }
    if ((rc = statuses(ve, nv, vst.data()))) return rc;
    std::vector<hc_sr_next_entry> list;
    std::vector<uint64_t> slot_of;  // the clique (< n_cliques) or n_cliques + vertex behind every listed entry
    for (uint64_t i = 0; i < nc; i++)  // writeSinglesToFile, :1142
        if (pst[i] == HC_SR_NEXT_KEPT && pe[i].kind == HC_SR_NEXT_SINGLE) list.push_back(pe[i]), slot_of.push_back(i);
    out->n_singles = list.size();
    for (uint64_t v = 0; v < nv; v++) {
        const uint32_t state = hc::mn::vertex_state(visited[v] != 0, vst[v], false, false, false, false);
        out->vertex_state[v] = state;
        visited[v] = state != HC_SR_MN_V_TRIVIAL;                                           // :1150, :1156
        if (state == HC_SR_MN_V_TRIVIAL) list.push_back(ve[v]), slot_of.push_back(nc + v);  // trivial_SR_vec, :1184-1216
        out->counts.n_dropped_short += state == HC_SR_MN_V_SHORT;
        out->counts.n_dropped_n_rate += state == HC_SR_MN_V_N_RATE;
        out->counts.n_bad += state == HC_SR_MN_V_BAD;
    }
    out->n_trivials = list.size() - out->n_singles;
    for (uint64_t i = 0; i < nc; i++) {  // writePairsToFile, :1233
        if (pst[i] == HC_SR_NEXT_KEPT && pe[i].kind == HC_SR_NEXT_PAIRED) list.push_back(pe[i]), slot_of.push_back(i);
        out->counts.n_dropped_empty += out->clique_kind[i] == HC_SR_MN_DROPPED_EMPTY;
        out->counts.n_dropped_n_rate += out->clique_kind[i] == HC_SR_MN_DROPPED_N_RATE;
        out->counts.n_bad += out->clique_kind[i] == HC_SR_MN_NONE;
        out->clique_new_id[i] = -1;
    }
    out->n_paired = list.size() - out->n_singles - out->n_trivials;
    out->n_srs = out->n_singles + out->n_paired;
    out->new_read_count = list.size();  // :1234
    // the ids and the tables
    for (uint64_t v = 0; v < nv; v++) {
        const uint32_t read = in->vertex_read[v];
        const uint32_t nm = read < n_reads ? read_first_seq[read + 1] - read_first_seq[read] : 0;
        hc_fno_read nd;
        memset(&nd, 0, sizeof nd);
        if (nm) {
            const uint32_t q = read_first_seq[read];
            nd.len1 = (uint32_t)(seq_off[q + 1] - seq_off[q]);
            nd.len2 = nm == 2 ? (uint32_t)(seq_off[q + 2] - seq_off[q + 1]) : 0;
            nd.paired = nm == 2;
        }
        nd.visited = visited[v];
        nd.orientation = in->vertex_fwd[v] ? 1 : 0;
        out->nodes[v] = nd;
    }
    // (the rows and the subread lists are written in two passes, singles then pairs, so that their offsets ascend with k)
    std::vector<uint64_t> sr_slot(out->n_srs);
    for (uint64_t pos = 0; pos < list.size(); pos++) {
        const uint64_t j = slot_of[pos];
        if (j >= nc) {
            out->nodes[j - nc].id = pos;  // nodes_to_new_IDs, :1219
            continue;
        }
        out->clique_new_id[j] = (int32_t)pos;
        const bool single = list[pos].kind == HC_SR_NEXT_SINGLE;
        const uint64_t k = single ? pos : pos - out->n_trivials;
        hc_fno_read sr;
        memset(&sr, 0, sizeof sr);
        sr.id = pos;
        sr.len1 = list[pos].len1;
        sr.len2 = single ? 0 : list[pos].len2;
        sr.paired = single ? 0 : 1;
        out->srs[k] = sr;
        out->sr_clique[k] = (uint32_t)j;
        sr_slot[k] = j;
    }
    uint64_t n_rows = 0, n_sub = 0;
    for (uint64_t k = 0; k < out->n_srs; k++) {
        const uint64_t i = sr_slot[k], a = in->clique_off[i], b = in->clique_off[i + 1];
        const int32_t op = out->overlap_pos[i];
        // the clique's vertices in ascending order (:658): the order `subreads` is in
        std::vector<uint32_t> sorted(in->clique_nodes + a, in->clique_nodes + b);
        std::sort(sorted.begin(), sorted.end());
        auto info_of = [&](uint32_t x, hc_sr_subread_info& s) {
            const auto it = std::lower_bound(sorted.begin(), sorted.end(), x);
            if (it == sorted.end() || *it != x) return false;
            s = in->subreads[a + (uint64_t)(it - sorted.begin())];
            return true;
        };
        out->subread_off[k] = n_sub;
        for (uint64_t j = 0; j < b - a; j++) {  // new_subreadMap, :915-925
            const hc_sr_subread_info s = in->subreads[a + j];
            out->subreads[n_sub++] = hc_fno_subread{sorted[j], s.index1, op >= 0 ? hc::mn::shift_index2(s.index2, op) : s.index2, s.startpos1, s.startpos2};
        }
        const hc_sr_layout L = in->layouts[in->first_layout[i]];
        out->clique_off[k] = n_rows;
        if (op < 0) {  // get_sorted_clique(0) / (1), :853, :864
            if (n_rows + L.n_members > 2 * n_items) return fail(me, HC_ERR_ARG, "the rows hold more than 2 N vertices: clique_nodes has no room for them");
            for (uint64_t m = 0; m < L.n_members; m++) out->clique_nodes[n_rows++] = in->member_vertex[L.first_member + m];
            continue;
        }
        // new_sorted_clique, :913-935: (vertex, index1) and, where index2 >= 0, (vertex, index2 + overlap_pos) in the documented order
        // among equal indexes — descending member position, index1 first — then a stable sort by index
        std::vector<std::pair<int32_t, uint32_t>> pairs;
        for (uint64_t m = L.n_members; m-- > 0;) {
            const uint32_t x = in->member_vertex[L.first_member + m];
            hc_sr_subread_info s;
            if (!info_of(x, s)) continue;
            pairs.push_back({s.index1, x});
            if (s.index2 >= 0) pairs.push_back({hc::mn::shift_index2(s.index2, op), x});
        }
        std::stable_sort(pairs.begin(), pairs.end(),
                         [](const std::pair<int32_t, uint32_t>& p, const std::pair<int32_t, uint32_t>& q) { return p.first < q.first; });
        if (n_rows + pairs.size() > 2 * n_items) return fail(me, HC_ERR_ARG, "the rows hold more than 2 N vertices: clique_nodes has no room for them");
        for (const auto& p : pairs) out->clique_nodes[n_rows++] = p.second;
    }
    out->clique_off[out->n_srs] = n_rows;
    out->subread_off[out->n_srs] = n_sub;
    // the store, :1142, :1231-1233
    hc_sr_next_counts cn;
    memset(&cn, 0, sizeof cn);
    out_seq_off[0] = 0;
    out_read_first_seq[0] = 0;
    std::vector<uint32_t> lst(list.size() ? list.size() : 1);
    rc = list.empty() ? HC_SR_NEXT_EMPTY
                      : hc_host_sr_next_reads(bases, quals, seq_off, read_first_seq, n_reads, kept_seq.data(), kept_qual.data(), n_kept_bytes, list.data(),
                                              list.size(), nullptr, nullptr, 0, &ns, tmp_id.data(), lst.data(), &cn, out_bases, out_quals, cap, n_bytes,
                                              out_seq_off, out_read_first_seq);
    out->counts.n_kept = cn.n_kept;
    out->counts.n_seq = cn.n_seq;
    out->counts.n_bytes = cn.n_bytes;
    if (!list.empty() && cn.n_kept != list.size()) return fail(me, HC_ERR_STATE, "an entry that passed its tests was dropped from the list");
    return rc;
}

extern "C" int hc_host_sr_clique_select(const uint64_t* clique_off, const uint32_t* clique_nodes, uint64_t n_cliques, uint64_t n_vertices,
                                        uint32_t min_clique_size, int remove_multi_occ, uint64_t* sel_off, uint32_t* sel_nodes, uint64_t* sel_index,
                                        uint64_t* n_selected, uint64_t* n_singletons) {
    const char* me = "hc_host_sr_clique_select";
    if (!clique_off || !sel_off || !n_selected || !n_singletons || (n_cliques && !sel_index)) return fail(me, HC_ERR_ARG, "null argument");
    if (clique_off[0] != 0) return fail(me, HC_ERR_ARG, "clique_off[0] is not 0");
    for (uint64_t i = 0; i < n_cliques; i++)
        if (clique_off[i + 1] < clique_off[i]) return fail(me, HC_ERR_ARG, "clique_off descends");
    const uint64_t n_items = clique_off[n_cliques];
    if (n_items && (!clique_nodes || !sel_nodes)) return fail(me, HC_ERR_ARG, "null argument");
    for (uint64_t j = 0; j < n_items; j++)
        if (clique_nodes[j] >= n_vertices) return fail(me, HC_ERR_ARG, "a vertex is not one of the graph's");
    std::vector<bool> used_nodes(n_vertices, false);  // :1055
    uint64_t n_sel = 0, n_out = 0, singleton_count = 0;
    sel_off[0] = 0;
    for (uint64_t i = 0; i < n_cliques; i++) {  // one line of cliques.txt, :1056
        std::vector<uint32_t> clique(clique_nodes + clique_off[i], clique_nodes + clique_off[i + 1]);
        if (remove_multi_occ) {  // filter out nodes that have occurred in previous cliques, :1065-1073
            std::vector<uint32_t> filtered_clique;
            for (uint32_t node : clique)
                if (!used_nodes[node]) filtered_clique.push_back(node);
            clique = filtered_clique;
        }
        if (clique.size() == 1) {  // :1075
            singleton_count++;
        } else if (clique.size() >= min_clique_size) {  // :1078
            for (uint32_t node : clique) {
                sel_nodes[n_out++] = node;
                used_nodes[node] = true;  // :1081-1083
            }
            sel_index[n_sel++] = i;
            sel_off[n_sel] = n_out;
        }
    }
    *n_selected = n_sel;
    *n_singletons = singleton_count;
    return HC_OK;
}
