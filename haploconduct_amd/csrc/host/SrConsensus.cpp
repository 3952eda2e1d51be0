// SrConsensus.cpp — host mirror of the super-read consensus (include/hcsr.h): SRBuilder::consensus / consensus_pos
// (reference src/SRBuilder.cpp:289-535) for a batch of layouts on plain base / quality arrays, and the layout of an edge merge
// between single-end reads (sort_vertices type 's', :33-285), and the mirrors of the edge merge on a graph: getEdgesForMerging
// (src/GraphAlgos.cpp:112-148), sort_vertices for a clique of two of every read type and calcSubreadInfo (:536-595), walked with a list
// as the reference walks them (the device: hc_sr_edge_kernels.hip).  Own implementation; it walks a layout column by column as the
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

int hc_host_graph_merge_pairs(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, uint32_t* pairs, uint64_t cap,
                              uint64_t* n_pairs) {
    if (!out_off || !n_pairs || (n_vertices && out_off[n_vertices] && !edges))
        return hc::set_last_error(HC_ERR_ARG, "hc_host_graph_merge_pairs: null argument");
    if (n_vertices >= (1ull << 32)) return hc::set_last_error(HC_ERR_ARG, "hc_host_graph_merge_pairs: more than 2^32 - 1 vertices");
    // getEdgesForMerging (src/GraphAlgos.cpp:112-148): bitvec, the lists in vertex order, the first unmarked outneighbor
    std::vector<uint8_t> bitvec(n_vertices, 0);
    std::vector<uint32_t> node_vec;
    for (uint64_t node = 0; node < n_vertices; node++) {
        if (bitvec[node]) continue;
        for (uint64_t k = out_off[node]; k < out_off[node + 1]; k++) {
            const uint64_t outneighbor = edges[k].v2;
            if (outneighbor >= n_vertices)
                return hc::set_last_error(HC_ERR_BAD_OVERLAP, "hc_host_graph_merge_pairs: record " + std::to_string(k) + " leaves the graph");
            if (!bitvec[outneighbor]) {
                node_vec.push_back((uint32_t)node);
                node_vec.push_back((uint32_t)outneighbor);
                bitvec[node] = 1;
                bitvec[outneighbor] = 1;
                break;
            }
        }
    }
    *n_pairs = node_vec.size() / 2;
    if (*n_pairs > cap || (*n_pairs && !pairs))
        return hc::set_last_error(HC_ERR_ARG, "hc_host_graph_merge_pairs: room for " + std::to_string(cap) + " pairs, " + std::to_string(*n_pairs) +
                                                  " needed (*n_pairs)");
    if (*n_pairs) memcpy(pairs, node_vec.data(), node_vec.size() * sizeof(uint32_t));
    return HC_OK;
}

namespace {

struct EdgeGraph {
    const hc_edge_rec* edges;
    const uint64_t* out_off;
    uint64_t V;
    const uint64_t* seq_off;
    const uint32_t* first;
    uint32_t n_reads;
    const uint32_t* vertex_read;
    const uint8_t* vertex_fwd;
    bool paired(uint32_t r) const { return first[r + 1] - first[r] == 2; }
    int64_t len(uint32_t r, uint32_t seq) const {  // Read::get_seq(seq).length()
        const uint32_t s = first[r] + (seq == 2 ? 1u : 0u);
        return (int64_t)(seq_off[s + 1] - seq_off[s]);
    }
    // OverlapGraph::getEdgeInfo, src/OverlapGraph.cpp:263-282
    const hc_edge_rec* edge_info(uint64_t v, uint64_t w) const {
        for (uint64_t k = out_off[v]; k < out_off[v + 1]; k++)
            if (edges[k].v2 == w) return &edges[k];
        for (uint64_t k = out_off[w]; k < out_off[w + 1]; k++)
            if (edges[k].v2 == v) return &edges[k];
        return nullptr;
    }
};

struct ListEntry {
    int64_t pos;
    uint64_t vertex;
    hc_sr_member m;
    int64_t len;
};

// sort_vertices (src/SRBuilder.cpp:33-285) for the clique {base_node, node}.  Returns HC_SR_EDGE_*; fills list and total_len.
uint32_t sort_two(const EdgeGraph& G, char type, uint64_t base_node, uint64_t node, std::vector<ListEntry>& list, int64_t& total_len) {
    list.clear();
    const uint32_t base_ID = G.vertex_read[base_node];
    ListEntry base{};
    base.vertex = base_node;
    base.m.read = base_ID;
    if (G.vertex_fwd[base_node]) {  // :47-61
        base.m.seq = type == 'l' ? 1 : type == 'r' ? 2 : 0;
        base.m.rev = 0;
    } else {  // :62-76
        base.m.seq = type == 'l' ? 2 : type == 'r' ? 1 : 0;
        base.m.rev = 1;
    }
    base.len = G.len(base_ID, base.m.seq);
    base.pos = 0;
    list.push_back(base);
    total_len = base.len;
    int64_t l_ext = 0, r_ext = 0;
    const hc_edge_rec* edge = G.edge_info(base_node, node);  // :92
    if (!edge) return HC_SR_EDGE_NO_EDGE;
    const bool current_ori = G.vertex_fwd[node] != 0;
    const uint32_t id1 = edge->read1, id2 = edge->read2;
    const char ord = (char)edge->ord;
    uint32_t current_id;
    if (id1 == base_ID) current_id = id2;  // :104-110
    else if (id2 == base_ID) current_id = id1;
    else return HC_SR_EDGE_READ_MISMATCH;
    if (current_id >= G.n_reads) return HC_SR_EDGE_BAD_VERTEX;
    char current_type = type;
    if (type == 's') current_type = G.paired(current_id) ? 'p' : 's';  // :114-122
    else if (!G.paired(current_id)) return HC_SR_EDGE_READ_MISMATCH;    // get_seq(1 | 2) of a single-end read, src/Read.h:145-149
    ListEntry cur{}, cur1{};
    cur.vertex = cur1.vertex = node;
    cur.m.read = cur1.m.read = current_id;
    cur.m.rev = cur1.m.rev = current_ori ? 0 : 1;
    int64_t new_pos = 0, new_pos1 = 0;
    if (current_type == 's') {  // :132-148
        const int64_t pos = edge->pos1;
        cur.m.seq = 0;
        new_pos = base_ID == id1 ? pos : -pos;
    } else if (current_type == 'l' || current_type == 'p') {  // :149-170
        const int64_t pos = edge->pos1;
        cur.m.seq = current_ori ? 1 : 2;
        new_pos = base_ID == id1 ? pos : -pos;
        if (current_type == 'p') {
            cur1 = cur;
            new_pos1 = new_pos;
        }
    }
    if (current_type == 'r' || current_type == 'p') {  // :171-188
        const int64_t pos = edge->pos2;
        cur.m.seq = current_ori ? 2 : 1;
        if (current_type == 'p' || (base_ID == id1 && ord == '1') || (base_ID == id2 && ord == '2')) new_pos = pos;
        else new_pos = -pos;
    }
    cur.len = G.len(current_id, cur.m.seq);
    auto insert = [&](ListEntry e, int64_t p) {  // :198-222
        size_t it = 0;
        while (it != list.size() && list[it].pos < p) it++;
        e.pos = p;
        list.insert(list.begin() + it, e);
    };
    if (current_type == 'p') {
        cur1.len = G.len(current_id, cur1.m.seq);
        insert(cur1, new_pos1);
    }
    insert(cur, new_pos);
    int64_t len1, len2;  // :225-240
    if (current_type == 'p') {
        if (new_pos < 0) return HC_SR_EDGE_PAIRED_NEG_POS;
        len1 = -new_pos1;
        len2 = cur.len + new_pos - base.len;
        const int64_t seq1_len2 = cur1.len + new_pos1 - base.len;
        if (seq1_len2 > len2) len2 = seq1_len2;
    } else {
        len1 = -new_pos;
        len2 = cur.len + new_pos - base.len;
    }
    if (len1 > l_ext) l_ext = len1;
    if (len2 > r_ext) r_ext = len2;
    total_len += l_ext + r_ext;  // :244
    if (total_len > INT32_MAX) return HC_SR_EDGE_BAD_GEOMETRY;
    if (!(total_len > list.back().pos)) return HC_SR_EDGE_BAD_GEOMETRY;  // :246
    const int64_t min = list.front().pos;  // :248-252
    if (min < 0)
        for (ListEntry& e : list) e.pos -= min;
    if (list.front().pos != 0 || list.front().len > total_len) return HC_SR_EDGE_BAD_GEOMETRY;  // :256, :259
    int64_t c_pos = 0;
    for (size_t i = 1; i < list.size(); i++) {  // :261-284
        const int64_t n_pos = list[i].pos;
        if (n_pos < 0 || c_pos > n_pos || n_pos > INT32_MAX || n_pos + list[i].len > total_len) return HC_SR_EDGE_BAD_GEOMETRY;
        c_pos = n_pos;
    }
    return HC_SR_EDGE_OK;
}

// calcSubreadInfo (src/SRBuilder.cpp:536-595); `info` is keyed by the pair's two vertices
void subread_info(int32_t trim_pos1, int32_t trim_pos2, const std::vector<ListEntry>& list1, const std::vector<ListEntry>& list2, uint64_t va,
                  hc_sr_subread_info* info) {
    bool present[2] = {false, false};
    for (const ListEntry& e : list1) {
        const int which = e.vertex == va ? 0 : 1;
        hc_sr_subread_info& s = info[which];
        const int32_t pos = (int32_t)e.pos;
        if (present[which]) {  // :544-558
            if (trim_pos1 > pos) {
                s.startpos2 = trim_pos1 - pos;
                s.index2 = 0;
            } else {
                s.startpos2 = 0;
                s.index2 = pos - trim_pos1;
            }
        } else {  // :559-572
            if (trim_pos1 > pos) {
                s.startpos1 = trim_pos1 - pos;
                s.index1 = 0;
            } else {
                s.startpos1 = 0;
                s.index1 = pos - trim_pos1;
            }
            s.index2 = -1;
            s.startpos2 = -1;
            present[which] = true;
        }
    }
    if (trim_pos2 >= 0) {  // :575-593
        for (const ListEntry& e : list2) {
            hc_sr_subread_info& s = info[e.vertex == va ? 0 : 1];
            const int32_t pos = (int32_t)e.pos;
            if (trim_pos2 > pos) {
                s.startpos2 = trim_pos2 - pos;
                s.index2 = 0;
            } else {
                s.startpos2 = 0;
                s.index2 = pos - trim_pos2;
            }
        }
    }
}

}  // namespace

int hc_host_sr_edge_merge_layouts(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, const uint64_t* seq_off,
                                  const uint32_t* read_first_seq, uint32_t n_reads, const uint32_t* pairs, uint64_t n_pairs,
                                  const uint32_t* vertex_read, const uint8_t* vertex_fwd, const hc_sr_settings* settings, uint32_t* pair_status,
                                  uint64_t* first_layout, hc_sr_layout* layouts, hc_sr_member* members, const int32_t* ret,
                                  hc_sr_subread_info* subreads) {
    const char* me = "hc_host_sr_edge_merge_layouts: ";
    if (!out_off || !seq_off || !read_first_seq || !settings || !first_layout || (n_vertices && (!vertex_read || !vertex_fwd)) ||
        (n_pairs && (!pairs || !pair_status || !layouts || !members)) || (n_vertices && out_off[n_vertices] && !edges) || (ret && n_pairs && !subreads))
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "null argument");
    if (settings->min_clique_size == 0)
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "min_clique_size == 0 sends a two-vertex clique through filter_subreads "
                                                                "(src/SRBuilder.cpp:721), which is not built");
    const EdgeGraph G{edges, out_off, n_vertices, seq_off, read_first_seq, n_reads, vertex_read, vertex_fwd};
    uint64_t n_layouts = 0, n_members = 0;
    std::vector<ListEntry> list1, list2;
    for (uint64_t i = 0; i < n_pairs; i++) {
        first_layout[i] = n_layouts;
        const uint64_t v = pairs[2 * i], w = pairs[2 * i + 1];
        uint32_t st = HC_SR_EDGE_OK;
        if (v >= n_vertices || w >= n_vertices || v == w || vertex_read[v] >= n_reads || vertex_read[w] >= n_reads) st = HC_SR_EDGE_BAD_VERTEX;
        const uint64_t va = std::min(v, w), vb = std::max(v, w);  // :658
        char type = 'p';
        int64_t len1 = 0, len2 = 0;
        if (st == HC_SR_EDGE_OK) {
            uint64_t base_node = va;  // :669-679
            for (uint64_t x : {va, vb})
                if (type == 'p' && !G.paired(vertex_read[x])) {
                    base_node = x;
                    type = 's';
                }
            if (type == 'p') {  // :691-698
                st = sort_two(G, 'l', va, vb, list1, len1);
                if (st == HC_SR_EDGE_OK) st = sort_two(G, 'r', va, vb, list2, len2);
            } else {
                st = sort_two(G, 's', base_node, base_node == va ? vb : va, list1, len1);
            }
        }
        pair_status[i] = st;
        if (subreads) subreads[2 * i] = subreads[2 * i + 1] = hc_sr_subread_info{-1, -1, -1, -1};
        if (st != HC_SR_EDGE_OK) continue;
        const uint64_t l0 = n_layouts;
        for (int k = 0; k < (type == 'p' ? 2 : 1); k++) {
            const std::vector<ListEntry>& L = k ? list2 : list1;
            layouts[n_layouts].first_member = n_members;
            layouts[n_layouts].n_members = (uint32_t)L.size();
            layouts[n_layouts].total_len = (int32_t)(k ? len2 : len1);
            for (const ListEntry& e : L) {
                hc_sr_member m = e.m;
                m.pos = (int32_t)e.pos;
                members[n_members++] = m;
            }
            n_layouts++;
        }
        if (ret && subreads) {
            if (type != 'p') list2.clear();
            subread_info(ret[l0], type == 'p' ? ret[l0 + 1] : -1, list1, list2, va, &subreads[2 * i]);
        }
    }
    first_layout[n_pairs] = n_layouts;
    return HC_OK;
}

}  // extern "C"
