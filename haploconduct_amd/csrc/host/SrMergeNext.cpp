// SrMergeNext.cpp — hc_host_sr_merge_next (include/hcsr.h): the host mirror of hc_sr_merge_next.  It walks the loops of
// SRBuilder::process_cliques (reference src/SRBuilder.cpp:978-1003) and mergeAlongEdges (:1260-1380) as they are written, one thread,
// over the mirrors of the steps in between: hc_host_sr_merge_self_overlaps for merge_self_overlap and hc_host_sr_next_reads for
// test_N_rate, get_len, the numbering and the bytes.  The expressions it shares with the device are those of hc_sr_merge_next.h.
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/hcsr.h"
#include "../hc_ctx.h"
#include "../hc_sr_merge_next.h"

namespace {

int fail(int status, const std::string& what) { return hc::set_last_error(status, std::string("hc_host_sr_merge_next: ") + what); }

}  // namespace

extern "C" int hc_host_sr_merge_next(const hc_settings* ec_settings, const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off,
                                     const uint32_t* read_first_seq, uint32_t n_reads, const uint8_t* cons_seq, const uint8_t* cons_qual,
                                     uint64_t n_cons, const hc_sr_merge_next_input* in, const hc_sr_merge_next_settings* st,
                                     hc_sr_merge_next_output* out, uint8_t* out_bases, uint8_t* out_quals, uint64_t cap, uint64_t* n_bytes,
                                     uint64_t* out_seq_off, uint32_t* out_read_first_seq) {
    if (!ec_settings || !in || !st || !out || !n_bytes || !out_seq_off || !out_read_first_seq || (n_cons && (!cons_seq || !cons_qual)) ||
        (n_reads && (!seq_off || !read_first_seq)))
        return fail(HC_ERR_ARG, "null argument");
    const uint64_t np = in->n_pairs, nv = in->n_vertices, n_slots = np + nv;
    if (n_slots >= (1ull << 31)) return fail(HC_ERR_ARG, "n_pairs + n_vertices is 2^31 or more");
    if ((np && (!in->pairs || !in->pair_status || !in->first_layout || !in->subreads || !out->pair_kind || !out->pair_new_id || !out->overlap_pos ||
                !out->self_score || !out->srs || !out->sr_pair || !out->clique_nodes || !out->subreads)) ||
        (nv && (!in->vertex_read || !in->vertex_fwd || !out->vertex_state || !out->nodes || !out->tips)) || !out->clique_off || !out->subread_off)
        return fail(HC_ERR_ARG, "null array");
    const uint64_t n_layouts = np ? in->first_layout[np] : 0;
    if (n_layouts > 2 * np || (n_layouts && (!in->layouts || !in->status || !in->out_off)) || (in->n_members && !in->members) || in->n_members > 6 * np)
        return fail(HC_ERR_ARG, "first_layout[n_pairs] exceeds 2 n_pairs, n_members exceeds 6 n_pairs, or the layouts are missing");
    const hc::mn::In I{in->pairs, in->pair_status, in->first_layout, in->layouts, in->members, in->status, in->out_off, in->subreads, in->vertex_read,
                       in->vertex_fwd, in->inclusions, in->tip_reads, np, n_layouts, in->n_members, nv, n_reads};
    out->n_srs = out->n_singles = out->n_trivials = out->n_paired = out->n_tips = out->n_self_merged = out->new_read_count = 0;
    out->ms_device = out->ms_copy = 0;
    memset(&out->counts, 0, sizeof out->counts);
    memset(&out->self_stats, 0, sizeof out->self_stats);
    *n_bytes = 0;

    // process_cliques, :978-1003: constructSuperread's result per pair, then merge_self_overlap for a paired one with two mates
    std::vector<hc_sr_next_entry> pe(np);
    std::vector<uint64_t> cand;
    std::vector<hc_sr_pair> self_pairs;
    for (uint64_t i = 0; i < np; i++) {
        uint32_t nc;
        hc::mn::pair_entry(I, i, pe[i], nc);
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
    std::vector<uint32_t> pst(np ? np : 1), vst(nv ? nv : 1);
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
    int rc = statuses(pe, np, pst.data());
    if (rc) return rc;
    // :1260-1277: the vertices of single_SR_vec's and paired_SR_vec's cliques
    std::vector<uint8_t> visited(nv ? nv : 1, 0);
    for (uint64_t i = 0; i < np; i++) {
        out->pair_kind[i] = hc::mn::pair_kind(pe[i].kind, pst[i], out->overlap_pos[i] >= 0);
        if (pst[i] != HC_SR_NEXT_KEPT) continue;
        visited[in->pairs[2 * i]] = 1;
        visited[in->pairs[2 * i + 1]] = 1;
    }
    // :1282-1373
    std::vector<hc_sr_next_entry> ve(nv);
    for (uint64_t v = 0; v < nv; v++) {
        const uint32_t read = in->vertex_read[v];
        const uint32_t nm = read < n_reads ? read_first_seq[read + 1] - read_first_seq[read] : 0;
        ve[v] = hc_sr_next_entry{0, 0, 0, 0, read, hc::mn::kNoEntry, 0, 0, (uint8_t)(in->vertex_fwd[v] ? 0 : 1)};
        if (!visited[v]) ve[v].kind = nm == 2 ? HC_SR_NEXT_TRIVIAL_PAIRED : HC_SR_NEXT_TRIVIAL;
    }
    if ((rc = statuses(ve, nv, vst.data()))) return rc;
    std::vector<hc_sr_next_entry> list;
    std::vector<uint64_t> slot_of;  // the pair (< n_pairs) or n_pairs + vertex behind every listed entry
    for (uint64_t i = 0; i < np; i++)  // writeSinglesToFile, :1280
        if (pst[i] == HC_SR_NEXT_KEPT && pe[i].kind == HC_SR_NEXT_SINGLE) list.push_back(pe[i]), slot_of.push_back(i);
    out->n_singles = list.size();
    for (uint64_t v = 0; v < nv; v++) {
        const uint32_t read = in->vertex_read[v];
        const bool tip = in->tip_reads && read < n_reads && in->tip_reads[read];
        const uint32_t state = hc::mn::vertex_state(visited[v] != 0, vst[v], st->ignore_inclusions != 0, in->inclusions && in->inclusions[v],
                                                    st->store_tips_separately != 0, tip);
        out->vertex_state[v] = state;
        visited[v] = state != HC_SR_MN_V_TRIVIAL;
        if (state == HC_SR_MN_V_INCLUSION || state == HC_SR_MN_V_TIP) out->tips[out->n_tips++] = (uint32_t)v;  // tips_vec, :1302, :1309
        if (state == HC_SR_MN_V_TRIVIAL) list.push_back(ve[v]), slot_of.push_back(np + v);               // trivial_SR_vec, :1335-1367
        out->counts.n_dropped_short += state == HC_SR_MN_V_SHORT;
        out->counts.n_dropped_n_rate += state == HC_SR_MN_V_N_RATE;
        out->counts.n_bad += state == HC_SR_MN_V_BAD;
    }
    out->n_trivials = list.size() - out->n_singles;
    for (uint64_t i = 0; i < np; i++) {  // writePairsToFile, :1378
        if (pst[i] == HC_SR_NEXT_KEPT && pe[i].kind == HC_SR_NEXT_PAIRED) list.push_back(pe[i]), slot_of.push_back(i);
        out->counts.n_dropped_empty += out->pair_kind[i] == HC_SR_MN_DROPPED_EMPTY;
        out->counts.n_dropped_n_rate += out->pair_kind[i] == HC_SR_MN_DROPPED_N_RATE;
        out->counts.n_bad += out->pair_kind[i] == HC_SR_MN_NONE;
        out->pair_new_id[i] = -1;
    }
    out->n_paired = list.size() - out->n_singles - out->n_trivials;
    out->n_srs = out->n_singles + out->n_paired;
    out->new_read_count = list.size();  // :1380
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
    uint64_t n_clique = 0;
    for (uint64_t pos = 0; pos < list.size(); pos++) {
        const uint64_t j = slot_of[pos];
        if (j >= np) {
            out->nodes[j - np].id = pos;  // nodes_to_new_IDs, :1370
            continue;
        }
        out->pair_new_id[j] = (int32_t)pos;
        const bool single = list[pos].kind == HC_SR_NEXT_SINGLE;
        const uint64_t k = single ? pos : pos - out->n_trivials;
        hc_fno_read sr;
        memset(&sr, 0, sizeof sr);
        sr.id = pos;
        sr.len1 = list[pos].len1;
        sr.len2 = single ? 0 : list[pos].len2;
        sr.paired = single ? 0 : 1;
        out->srs[k] = sr;
        out->sr_pair[k] = (uint32_t)j;
        uint64_t clique[4];
        hc_fno_subread sub[2];
        memset(sub, 0, sizeof sub);
        const uint32_t n = hc::mn::sr_tables(I, j, out->overlap_pos[j], clique, sub);
        out->clique_off[k] = n_clique;
        for (uint32_t a = 0; a < n; a++) out->clique_nodes[n_clique++] = clique[a];
        out->subread_off[k] = 2 * k;
        out->subreads[2 * k] = sub[0];
        out->subreads[2 * k + 1] = sub[1];
    }
    out->clique_off[out->n_srs] = n_clique;
    out->subread_off[out->n_srs] = 2 * out->n_srs;
    // the store, :1280, :1377-1378
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
    if (!list.empty() && cn.n_kept != list.size()) return fail(HC_ERR_STATE, "an entry that passed its tests was dropped from the list");
    return rc;
}
