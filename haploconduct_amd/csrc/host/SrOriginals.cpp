// SrOriginals.cpp — hc_host_sr_originals_next, hc_host_sr_originals_text and hc_host_sr_originals_parse (include/hcsr.h): the host mirrors
// of the original-read index maps.  The first walks constructSuperread's loop over a clique's vertices and their originals (reference
// src/SRBuilder.cpp:750-806) with merge_self_overlap's shift (:938-949), and the trivial super-reads' copies (:1161-1216, :1312-1369), as
// they are written — a map per new read, a vertex at a time, an original an earlier vertex supplied skipped — and then sorts every map by
// id; the expressions are hc_sr_originals.h's, shared with the device.  The second is the writers' loop (:1449-1463), the third the else
// branch of OverlapGraph::buildOriginalsDict (src/OverlapGraph.cpp:807-838).  Also the argument checks the device call shares.
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../../include/hcsr.h"
#include "../hc_ctx.h"
#include "../hc_sr_originals.h"

namespace hc {
namespace orig {

const char* check_dict(const uint64_t* off, const hc_sr_original* entries, uint64_t n_reads) {
    if (!off) return "null orig_off";
    if (n_reads >= (1ull << 31)) return "2^31 reads or more";
    if (off[0] != 0) return "orig_off[0] is not 0";
    for (uint64_t r = 0; r < n_reads; r++)
        if (off[r + 1] < off[r]) return "orig_off descends";
    const uint64_t ne = off[n_reads];
    if (ne >= (1ull << 31)) return "2^31 entries or more";
    if (ne && !entries) return "null entries";
    for (uint64_t r = 0; r < n_reads; r++)
        for (uint64_t k = off[r]; k < off[r + 1]; k++) {
            if (k > off[r] && entries[k].id <= entries[k - 1].id) return "the ids of a read do not strictly ascend";
            if (entries[k].paired > 1 || entries[k].forward > 1) return "paired or forward above 1";
        }
    return nullptr;
}

const char* check_input(const hc_sr_originals_input* in, const hc_sr_originals_output* out, const uint64_t* dict_off, uint64_t dict_reads, uint64_t* n_cand) {
    const uint64_t nc = in->n_cliques, ns = in->n_srs, nv = in->n_vertices, n_new = in->new_read_count;
    if (n_new >= (1ull << 31) || nc >= (1ull << 31) || nv >= (1ull << 31) || ns > nc) return "new_read_count, n_cliques or n_vertices is 2^31 or more, or n_srs exceeds n_cliques";
    if (!out->orig_off || (n_new && !out->status)) return "null output array";
    if (nc && (!in->kind || !in->new_id || !in->overlap_pos || !in->first_layout)) return "null per-clique array";
    if (ns && (!in->sr_clique || !in->subread_off)) return "null per-super-read array";
    if (nv && (!in->vertex_state || !in->nodes || !in->vertex_read || !in->vertex_fwd)) return "null per-vertex array";
    for (uint64_t c = 0; c < nc; c++)
        if (in->first_layout[c + 1] < in->first_layout[c]) return "first_layout descends";
    const uint64_t n_layouts = nc ? in->first_layout[nc] : 0;
    if (n_layouts > 2 * nc || (n_layouts && !in->layouts)) return "first_layout[n_cliques] exceeds 2 n_cliques, or the layouts are missing";
    if (ns && in->subread_off[0] != 0) return "subread_off[0] is not 0";
    for (uint64_t k = 0; k < ns; k++)
        if (in->subread_off[k + 1] < in->subread_off[k]) return "subread_off descends";
    const uint64_t n_sub = ns ? in->subread_off[ns] : 0;
    if (n_sub >= (1ull << 31) || n_sub + nv >= (1ull << 31)) return "2^31 sources or more";
    if (n_sub && !in->subreads) return "null subreads";
    uint64_t total = 0;
    for (uint64_t k = 0; k < ns; k++) {
        const uint64_t c = in->sr_clique[k];
        if (c >= nc) return "sr_clique names no clique";
        if (in->new_id[c] < 0 || (uint64_t)in->new_id[c] >= n_new) return "a super-read's new id is not below new_read_count";
        for (uint64_t j = in->subread_off[k]; j < in->subread_off[k + 1]; j++) {
            const uint64_t v = in->subreads[j].node;
            if (v >= nv) return "a subread row names no vertex";
            if (in->vertex_read[v] >= dict_reads) return "vertex_read of a super-read's vertex is no read of the kept dict";
            if (dict_off) total += dict_off[in->vertex_read[v] + 1] - dict_off[in->vertex_read[v]];
        }
    }
    for (uint64_t v = 0; v < nv; v++) {
        if (in->vertex_state[v] != HC_SR_MN_V_TRIVIAL) continue;
        if (in->nodes[v].id >= n_new) return "a trivial's new id is not below new_read_count";
        if (in->vertex_read[v] >= dict_reads) return "vertex_read of a trivial is no read of the kept dict";
        if (dict_off) total += dict_off[in->vertex_read[v] + 1] - dict_off[in->vertex_read[v]];
    }
    if (total >= (1ull << 31)) return "2^31 candidate entries or more";
    if (n_cand) *n_cand = total;
    return nullptr;
}

}  // namespace orig
}  // namespace hc

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

typedef std::map<uint32_t, hc_sr_original> Map;  // (the reference's unordered_map, read out in ascending id)

struct NewRead {
    Map map;
    uint32_t bits = 0;
};

// constructSuperread, :750-806, and merge_self_overlap, :938-949, for super-read k
void super_read(const uint64_t* off, const hc_sr_original* entries, const hc_sr_originals_input* in, uint64_t k, NewRead& R) {
    const uint64_t c = in->sr_clique[k];
    const int32_t len2 = hc::orig::len2_of(in->first_layout, in->layouts, c);
    for (uint64_t j = in->subread_off[k]; j < in->subread_off[k + 1]; j++) {  // for (auto node_it : clique), :752
        const hc_fno_subread row = in->subreads[j];
        const uint64_t v = row.node;
        const uint32_t sub_id = in->vertex_read[v];
        const hc::orig::Source s = hc::orig::sr_source(row, in->nodes[v], in->vertex_fwd[v], in->kind[c], in->overlap_pos[c], len2, in->first_it);
        for (uint64_t a = off[sub_id]; a < off[sub_id + 1]; a++) {  // for (auto it : subreads), :760
            hc_sr_original e = entries[a];
            if (R.map.find(e.id) != R.map.end()) continue;  // already inserted by another node, :762
            const uint32_t b = hc::orig::transform(s, e);
            R.bits |= b;
            R.map.insert(std::make_pair(e.id, e));
        }
    }
}

// :1161-1216, :1312-1369 for trivial vertex v
void trivial(const uint64_t* off, const hc_sr_original* entries, const hc_sr_originals_input* in, uint64_t v, NewRead& R) {
    const uint32_t id = in->vertex_read[v];
    if (off[id + 1] == off[id]) R.bits |= hc::orig::kBitEmpty;  // assert (subreads.size() > 0)
    const hc::orig::Source s = hc::orig::trivial_source(in->nodes[v], in->vertex_fwd[v]);
    for (uint64_t a = off[id]; a < off[id + 1]; a++) {
        hc_sr_original e = entries[a];
        R.bits |= hc::orig::transform(s, e);
        R.map.insert(std::make_pair(e.id, e));
    }
}

}  // namespace

extern "C" int hc_host_sr_originals_next(const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads, const hc_sr_originals_input* in,
                                         hc_sr_originals_output* out, hc_sr_original* out_entries, uint64_t cap, uint32_t n_threads) {
    const char* me = "hc_host_sr_originals_next";
    if (!orig_off || !in || !out) return fail(me, HC_ERR_ARG, "null argument");
    out->n_entries = out->n_failed = 0;
    out->ms_device = out->ms_copy = 0;
    if (const char* what = hc::orig::check_dict(orig_off, entries, n_reads)) return fail(me, HC_ERR_ARG, what);
    uint64_t n_cand = 0;
    if (const char* what = hc::orig::check_input(in, out, orig_off, n_reads, &n_cand)) return fail(me, HC_ERR_ARG, what);
    const uint64_t ns = in->n_srs, nv = in->n_vertices, n_new = in->new_read_count;
    // the work items in any order: a new read's map is filled by the items that name it, a lock-free split needs each new read in one
    // thread — the items are dealt out by new id
    std::vector<NewRead> reads(n_new);
    const uint32_t nt = std::max<uint32_t>(1, std::min<uint32_t>(n_threads, 64));
    auto work = [&](uint32_t t) {
        for (uint64_t k = 0; k < ns; k++) {
            const uint64_t id = (uint64_t)in->new_id[in->sr_clique[k]];
            if (id % nt == t) super_read(orig_off, entries, in, k, reads[id]);
        }
        for (uint64_t v = 0; v < nv; v++) {
            if (in->vertex_state[v] != HC_SR_MN_V_TRIVIAL) continue;
            const uint64_t id = in->nodes[v].id;
            if (id % nt == t) trivial(orig_off, entries, in, v, reads[id]);
        }
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < nt; t++) pool.emplace_back(work, t);
        for (std::thread& th : pool) th.join();
    }
    uint64_t total = 0, n_failed = 0;
    for (uint64_t r = 0; r < n_new; r++) {
        out->orig_off[r] = total;
        out->status[r] = hc::orig::status_of(reads[r].bits);
        if (out->status[r] != HC_SR_ORIG_OK) {
            n_failed++;
            continue;
        }
        total += reads[r].map.size();
    }
    out->orig_off[n_new] = total;
    out->n_entries = total;
    out->n_failed = n_failed;
    if (total > cap || (total && !out_entries)) return fail(me, HC_ERR_ARG, "out_entries is missing or too small (n_entries is filled)");
    for (uint64_t r = 0; r < n_new; r++) {
        if (out->status[r] != HC_SR_ORIG_OK) continue;
        uint64_t at = out->orig_off[r];
        for (const auto& it : reads[r].map) out_entries[at++] = it.second;
    }
    return n_failed ? HC_SR_ORIG_SOME_FAILED : HC_OK;
}

extern "C" int hc_host_sr_originals_text(const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads, char* text, uint64_t cap,
                                         uint64_t* n_bytes) {
    const char* me = "hc_host_sr_originals_text";
    if (!orig_off || !n_bytes) return fail(me, HC_ERR_ARG, "null argument");
    *n_bytes = 0;
    if (const char* what = hc::orig::check_dict(orig_off, entries, n_reads)) return fail(me, HC_ERR_ARG, what);
    uint64_t total = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        total += hc::orig::dec_u32((uint32_t)r) + 1;
        for (uint64_t a = orig_off[r]; a < orig_off[r + 1]; a++) total += hc::orig::entry_chars(entries[a]);
    }
    *n_bytes = total;
    if (total > cap || (total && !text)) return fail(me, HC_ERR_ARG, "text is missing or too small (n_bytes is filled)");
    char* p = text;
    for (uint64_t r = 0; r < n_reads; r++) {  // originals << ID; per entry ...; originals << "\n", :1450-1463
        p = hc::orig::put_u32(p, (uint32_t)r);
        for (uint64_t a = orig_off[r]; a < orig_off[r + 1]; a++) p = hc::orig::put_entry(p, entries[a]);
        *p++ = '\n';
    }
    return HC_OK;
}

namespace {

// std::stol / str_to_read_id on a whole token: optional sign, digits, nothing else
bool whole_number(const char* b, const char* e, bool may_be_negative, int64_t lo, int64_t hi, int64_t& v) {
    bool neg = false;
    if (b < e && (*b == '-' || *b == '+')) {
        neg = *b == '-';
        if (neg && !may_be_negative) return false;
        b++;
    }
    if (b == e || e - b > 18) return false;
    int64_t x = 0;
    for (; b < e; b++) {
        if (*b < '0' || *b > '9') return false;
        x = x * 10 + (*b - '0');
    }
    v = neg ? -x : x;
    return v >= lo && v <= hi;
}

}  // namespace

extern "C" int hc_host_sr_originals_parse(const char* text, uint64_t n_bytes, uint64_t* orig_off, uint64_t cap_reads, hc_sr_original* entries,
                                          uint64_t cap_entries, uint64_t* n_reads, uint64_t* n_entries, uint64_t* bad_line) {
    const char* me = "hc_host_sr_originals_parse";
    if ((n_bytes && !text) || !n_reads || !n_entries) return fail(me, HC_ERR_ARG, "null argument");
    *n_reads = *n_entries = 0;
    if (bad_line) *bad_line = 0;
    std::map<uint32_t, Map> dict;  // original_ID_dict
    const char *p = text, *end = text + n_bytes;
    uint64_t line_no = 0;
    auto bad = [&](const char* what) {
        if (bad_line) *bad_line = line_no;
        return fail(me, HC_ERR_FORMAT, std::string(what) + " in line " + std::to_string(line_no));
    };
    for (; p < end; line_no++) {  // while (getline(originals, line)), :807
        const char* eol = (const char*)memchr(p, '\n', end - p);
        if (!eol) eol = end;
        const char* q = (const char*)memchr(p, '\t', eol - p);  // getline(ss, readID, '\t'), :809
        const char* id_end = q ? q : eol;
        int64_t id = 0;
        if (!whole_number(p, id_end, false, 0, INT32_MAX, id)) return bad("a read id that is no number below 2^31");
        Map m;
        const char* f = q ? q + 1 : eol;
        while (f < eol) {  // while (getline(ss, info, '\t')), :812
            const char* fe = (const char*)memchr(f, '\t', eol - f);
            if (!fe) fe = eol;
            // boost::algorithm::split(tmp_vec, info, is_any_of(":,"), token_compress_on), :815: adjacent separators are one
            std::vector<std::pair<const char*, const char*>> tok;
            const char* tb = f;
            for (const char* x = f;; x++) {
                if (x == fe || *x == ':' || *x == ',') {
                    tok.push_back(std::make_pair(tb, x));
                    if (x == fe) break;
                    while (x + 1 < fe && (x[1] == ':' || x[1] == ',')) x++;
                    tb = x + 1;
                }
            }
            if (tok.size() != 4 && tok.size() != 6) return bad("a field of another token count than 4 or 6");  // the assert of :816
            hc_sr_original e;
            memset(&e, 0, sizeof e);
            int64_t v = 0;
            if (!whole_number(tok[0].first, tok[0].second, false, 0, UINT32_MAX, v)) return bad("an original id that is no number below 2^32");
            e.id = (uint32_t)v;
            e.forward = tok[1].second - tok[1].first == 1 && *tok[1].first == '+';  // (tmp_vec[1] == "+"), :819
            const bool paired = tok.size() == 6;
            e.paired = paired;
            if (!whole_number(tok[2].first, tok[2].second, true, INT32_MIN, INT32_MAX, v)) return bad("an index1 that is no int32");
            e.index1 = (int32_t)v;
            if (paired) {
                if (!whole_number(tok[3].first, tok[3].second, true, INT32_MIN, INT32_MAX, v)) return bad("an index2 that is no int32");
                e.index2 = (int32_t)v;
            }
            if (!whole_number(tok[paired ? 4 : 3].first, tok[paired ? 4 : 3].second, false, 0, INT32_MAX, v)) return bad("a len1 that is no length");
            e.len1 = (uint32_t)v;
            if (paired) {
                if (!whole_number(tok[5].first, tok[5].second, false, 0, INT32_MAX, v)) return bad("a len2 that is no length");
                e.len2 = (uint32_t)v;
            }
            m.insert(std::make_pair(e.id, e));  // originals_map.insert: the first entry of an id stays, :832
            f = fe < eol ? fe + 1 : eol;
        }
        dict.insert(std::make_pair((uint32_t)id, std::move(m)));  // original_ID_dict.insert: the first line of an id stays, :835
        p = eol < end ? eol + 1 : end;
    }
    const uint64_t nr = dict.empty() ? 0 : (uint64_t)dict.rbegin()->first + 1;
    uint64_t ne = 0;
    for (const auto& it : dict) ne += it.second.size();
    *n_reads = nr;
    *n_entries = ne;
    if (!orig_off || cap_reads < nr || cap_entries < ne || (ne && !entries)) return fail(me, HC_ERR_ARG, "a buffer is missing or too small (the sizes are filled)");
    uint64_t at = 0, r = 0;
    for (const auto& it : dict) {
        for (; r <= it.first; r++) orig_off[r] = at;
        for (const auto& e : it.second) entries[at++] = e.second;
    }
    for (; r <= nr; r++) orig_off[r] = at;
    return HC_OK;
}
