// SrConsensus.cpp — host mirror of the super-read consensus (include/hcsr.h): SRBuilder::consensus / consensus_pos
// (reference src/SRBuilder.cpp:289-535) for a batch of layouts on plain base / quality arrays, and the layout of an edge merge
// between single-end reads (sort_vertices type 's', :33-285).  Own implementation; it walks a layout column by column as the
// reference does, so that the device's closed forms (hc_sr_kernels.hip) have something independent to be compared with.
#include "SrConsensus.h"

#include "InBlocks.h"

namespace {
using namespace hc;

struct Reads {
    const uint8_t *bases, *quals;
    const uint64_t* seq_off;
    const uint32_t* first;
    uint32_t n_reads;
};

struct MemberView {
    const uint8_t *b, *q;  // first base / quality of the stored (forward) sequence
    uint32_t len;
    bool rev;
    // base code (SrCodes.h) and quality byte at position i of the oriented sequence (Read.h: get_rev_comp / get_rev_phred)
    inline void at(uint32_t i, uint32_t& code, uint8_t& qual) const {
        const uint32_t j = rev ? len - 1 - i : i;
        code = code_of(b[j]);
        if (rev && code < 4) code = 3 - code;
        qual = q[j];
    }
};

// what hc_sr_consensus refuses per layout (hcsr.h: HC_SR_BAD_LAYOUT); fills `mv`
bool check_layout(const Reads& R, const hc_sr_layout& L, const hc_sr_member* members, uint64_t n_members, std::vector<MemberView>& mv) {
    mv.clear();
    if (L.n_members == 0 || L.first_member > n_members || L.n_members > n_members - L.first_member || L.total_len < 0) return false;
    int32_t prev = 0;
    for (uint32_t i = 0; i < L.n_members; i++) {
        const hc_sr_member& m = members[L.first_member + i];
        if (m.read >= R.n_reads || m.rev > 1 || m.seq > 2) return false;
        const uint32_t f = R.first[m.read], k = R.first[m.read + 1] - f;
        if (k == 1 ? m.seq != 0 : m.seq == 0) return false;  // asserts of src/Read.h:145-149
        const uint32_t s = f + (m.seq == 2 ? 1u : 0u);
        const uint64_t len = R.seq_off[s + 1] - R.seq_off[s];
        if (i == 0 ? m.pos != 0 : m.pos < prev) return false;
        if (len == 0 || (uint64_t)m.pos + len > (uint64_t)L.total_len) return false;
        prev = m.pos;
        mv.push_back(MemberView{R.bases + R.seq_off[s], R.quals + R.seq_off[s], (uint32_t)len, m.rev != 0});
    }
    return true;
}

// consensus (:413-535) for one layout.  seq / qual receive the bytes; returns the status, *ret the return value.
uint32_t one_layout(const hc_sr_layout& L, const hc_sr_member* mem, const std::vector<MemberView>& mv, const hc_sr_settings& st, const double* t_same,
                    const double* t_other, std::vector<uint8_t>& seq, std::vector<uint8_t>& qual, int32_t* ret) {
    const uint32_t n = L.n_members;
    seq.clear();
    qual.clear();
    const uint32_t minimum_support = st.subreads_needed ? 2u : st.min_clique_size;  // :421-427
    int32_t trim_pos = 0;
    if (st.error_correction) {  // :430-447
        uint32_t current_support = 1, it = 0;
        while (current_support < minimum_support && it != n) {
            current_support++;
            it++;
        }
        if (it == n) {
            *ret = -1;
            return HC_SR_NO_SUPPORT;
        }
        trim_pos = mem[it].pos;
    }
    std::vector<uint8_t> active(n, 0);
    std::vector<uint32_t> active_pos(n);
    uint32_t n_active = 0;
    for (uint32_t i = 0; i < n; i++) active_pos[i] = mem[i].pos < trim_pos ? (uint32_t)(trim_pos - mem[i].pos) : 0u;  // :452-459
    uint32_t next = 0;  // pos_it
    bool prefix_removed = false, bad_symbol = false;
    *ret = trim_pos;
    for (int32_t current_pos = 0; current_pos < L.total_len; current_pos++) {
        while (next != n && current_pos == mem[next].pos) {  // :468-472
            if (!active[next]) n_active++;
            active[next] = 1;
            next++;
        }
        if (st.error_correction && n_active < minimum_support) {  // :479-486
            if (next == n) break;
            else if (!prefix_removed) continue;
        }
        prefix_removed = true;
        sr::Sums sums;
        uint32_t k = 0;
        for (uint32_t i = 0; i < n; i++) {  // :488-506
            if (!active[i]) continue;
            const uint32_t pos = active_pos[i];
            if (pos >= mv[i].len) {
                seq.clear();
                qual.clear();
                *ret = 0;
                return HC_SR_MEMBER_SHORT;
            }
            uint32_t code;
            uint8_t q;
            mv[i].at(pos, code, q);
            if (code > 4 || q < 33 || q > 127) {  // the reference's asserts (:307, :340); the store's invalid symbols
                bad_symbol = true;
                code = 4;
                q = 33;
            }
            sums.add(code, t_same[q - 33], t_other[q - 33]);
            k++;
            if (pos + 1 < mv[i].len) active_pos[i] = pos + 1;
            else {
                active[i] = 0;
                n_active--;
            }
        }
        if (k == 0) {  // :507-510
            seq.clear();
            qual.clear();
            *ret = 0;
            return HC_SR_UNCOVERED;
        }
        uint8_t o[2];
        if (!sr::finish(sums.s[0], sums.s[1], sums.s[2], sums.s[3], k, st.min_qual, o)) {  // :527-532
            seq.clear();
            qual.clear();
            if (bad_symbol) break;
            return HC_SR_NAN;
        }
        seq.push_back(o[0]);
        qual.push_back(o[1]);
    }
    if (bad_symbol) {
        seq.clear();
        qual.clear();
        *ret = 0;
        return HC_SR_BAD_SYMBOL;
    }
    return HC_SR_OK;
}

}  // namespace

extern "C" {

int hc_host_sr_column(const uint8_t* nucleotides, const uint8_t* qualities, uint32_t n, double min_qual, uint8_t* out) {
    if (!out || (n && (!nucleotides || !qualities))) return hc::set_last_error(HC_ERR_ARG, "hc_host_sr_column: null"), 0;
    sr::Sums sums;
    for (uint32_t i = 0; i < n; i++) {
        double a, b;
        sr::terms((int)qualities[i] - 33, a, b);
        sums.add(code_or_n(nucleotides[i]), a, b);
    }
    return sr::finish(sums.s[0], sums.s[1], sums.s[2], sums.s[3], n, min_qual, out);
}

int hc_host_sr_table(double min_qual, uint32_t n_q, uint8_t* table) {
    if (!table || n_q > 95) return hc::set_last_error(HC_ERR_ARG, "hc_host_sr_table: null table or n_q > 95");
    std::vector<uint32_t> qs(n_q);
    for (uint32_t q = 0; q < n_q; q++) qs[q] = q;
    sr::build_table(min_qual, qs, table);
    return HC_OK;
}

int hc_host_sr_consensus(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq, uint32_t n_reads,
                         const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members, uint64_t n_members,
                         const hc_sr_settings* settings, int32_t* ret, uint32_t* status, uint64_t* out_off, uint8_t* cons_seq, uint8_t* cons_qual,
                         uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats) {
    if (!seq_off || !read_first_seq || !settings || !ret || !status || !out_off || !n_bytes || (n_layouts && !layouts) || (n_members && !members))
        return hc::set_last_error(HC_ERR_ARG, "hc_host_sr_consensus: null argument");
    if (!(settings->min_qual == settings->min_qual)) return hc::set_last_error(HC_ERR_ARG, "hc_host_sr_consensus: min_qual is NaN");
    const Reads R{bases, quals, seq_off, read_first_seq, n_reads};
    double t_same[sr::kQDim], t_other[sr::kQDim];
    for (uint32_t q = 0; q < sr::kQDim; q++) sr::terms((int)q, t_same[q], t_other[q]);
    // every thread takes blocks of layouts and keeps their bytes; the packed buffer is filled once the offsets are known
    struct Piece {
        std::vector<uint8_t> seq, qual;
    };
    const uint64_t block = 256, n_blocks = (n_layouts + block - 1) / block;
    std::vector<Piece> pieces(n_blocks);
    std::vector<uint32_t> lens(n_layouts);
    in_blocks(n_layouts, block, settings->n_threads, [&](uint64_t l0, uint64_t l1) {
        std::vector<MemberView> mv;
        std::vector<uint8_t> s, q;
        Piece& P = pieces[l0 / block];
        for (uint64_t l = l0; l < l1; l++) {
            if (!check_layout(R, layouts[l], members, n_members, mv)) {
                ret[l] = 0;
                status[l] = HC_SR_BAD_LAYOUT;
                lens[l] = 0;
                continue;
            }
            status[l] = one_layout(layouts[l], members + layouts[l].first_member, mv, *settings, t_same, t_other, s, q, &ret[l]);
            lens[l] = (uint32_t)s.size();
            P.seq.insert(P.seq.end(), s.begin(), s.end());
            P.qual.insert(P.qual.end(), q.begin(), q.end());
        }
    });
    uint64_t total = 0;
    for (uint64_t l = 0; l < n_layouts; l++) {
        out_off[l] = total;
        total += lens[l];
    }
    out_off[n_layouts] = total;
    *n_bytes = total;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->n_columns = total;
    }
    if (int rc = sr::check_room("hc_host_sr_consensus", "cons_seq / cons_qual", "n_bytes", total, cap, cons_seq, cons_qual)) return rc;
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (pieces[b].seq.empty()) continue;
        memcpy(cons_seq + out_off[b * block], pieces[b].seq.data(), pieces[b].seq.size());
        memcpy(cons_qual + out_off[b * block], pieces[b].qual.data(), pieces[b].qual.size());
    }
    return HC_OK;
}

int hc_host_sr_edge_layouts(const hc_edge_rec* edges, uint64_t n_edges, const uint32_t* seq_len_by_read, const uint8_t* paired, uint32_t n_reads,
                            hc_sr_layout* layouts, hc_sr_member* members, uint64_t* first_bad) {
    if ((n_edges && (!edges || !layouts || !members)) || !seq_len_by_read)
        return hc::set_last_error(HC_ERR_ARG, "hc_host_sr_edge_layouts: null argument");
    for (uint64_t i = 0; i < n_edges; i++) {
        const hc_edge_rec& e = edges[i];
        const bool ok = e.read1 < n_reads && e.read2 < n_reads && e.read1 != e.read2 && !(paired && (paired[e.read1] || paired[e.read2]));
        if (!ok) {
            if (first_bad) *first_bad = i;
            return hc::set_last_error(HC_ERR_BAD_OVERLAP, "hc_host_sr_edge_layouts: edge " + std::to_string(i) +
                                                              " names a paired read, a read out of range or one read twice");
        }
        // base_node = the smaller vertex; base_ID == id1 exactly when that is the edge's first vertex (:43, :95-104)
        const bool base_is_1 = e.v1 < e.v2;
        const uint32_t base_read = base_is_1 ? e.read1 : e.read2, other_read = base_is_1 ? e.read2 : e.read1;
        const uint8_t base_rev = (base_is_1 ? e.ori1 : e.ori2) ? 0 : 1, other_rev = (base_is_1 ? e.ori2 : e.ori1) ? 0 : 1;
        const int64_t base_len = seq_len_by_read[base_read], other_len = seq_len_by_read[other_read];
        const int64_t new_pos = base_is_1 ? (int64_t)e.pos1 : -(int64_t)e.pos1;  // :143-148
        const int64_t l_ext = std::max<int64_t>(0, -new_pos), r_ext = std::max<int64_t>(0, other_len + new_pos - base_len);  // :236-243
        const int64_t total_len = base_len + l_ext + r_ext;
        if (total_len > INT32_MAX) {
            if (first_bad) *first_bad = i;
            return hc::set_last_error(HC_ERR_BAD_OVERLAP, "hc_host_sr_edge_layouts: total_len does not fit an int");
        }
        hc_sr_member mb{}, mo{};
        mb.read = base_read;
        mb.rev = base_rev;
        mo.read = other_read;
        mo.rev = other_rev;
        // the other member goes in front of the first entry that is not smaller (:213-221), then all shift by -min (:247-250)
        const bool other_first = new_pos <= 0;
        mb.pos = (int32_t)(new_pos < 0 ? -new_pos : 0);
        mo.pos = (int32_t)(new_pos < 0 ? 0 : new_pos);
        members[2 * i] = other_first ? mo : mb;
        members[2 * i + 1] = other_first ? mb : mo;
        layouts[i].first_member = 2 * i;
        layouts[i].n_members = 2;
        layouts[i].total_len = (int32_t)total_len;
    }
    return HC_OK;
}

}  // extern "C"
