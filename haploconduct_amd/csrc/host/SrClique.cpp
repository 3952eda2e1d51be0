// SrClique.cpp — the host mirror of hc_sr_clique_merge (include/hcsr.h): constructSuperread for a clique of any size (reference
// src/SRBuilder.cpp:654-748) up to and behind consensus().  It walks the reference's loops as written: sort_vertices (:33-285) inserts into
// std::lists, filter_subreads (:597-651) keeps a std::set of selected vertices and calls std::sort with the reference's comparator on a
// vector in list order — built with the same libstdc++ as the golden probe, that IS the reference's order among ties — and
// calcSubreadInfo (:536-595) fills a map.  Beside the selection it reports, by the rule of SrCliqueFilter.h, whether the selection could
// depend on that order at all.
#include <algorithm>
#include <climits>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/hcsr.h"
#include "SrCliqueFilter.h"
#include "api_helpers.h"

namespace {

using hc::srclique::GroupStep;

struct Graph {
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

struct Entry {
    hc_sr_member m;
    int64_t len;
};

struct Lists {  // pos_list, seq_list / qual_list (as members), sorted_vertices
    std::list<int64_t> pos;
    std::list<Entry> seq;
    std::list<uint64_t> sorted_vertices;
    int64_t total_len = 0;
    void clear() {
        pos.clear();
        seq.clear();
        sorted_vertices.clear();
        total_len = 0;
    }
};

// sort_vertices (src/SRBuilder.cpp:33-285).  Returns HC_SR_EDGE_*.
uint32_t sort_vertices(const Graph& G, const std::vector<uint64_t>& vertices, char type, uint64_t base_node, Lists& L) {
    L.clear();
    const uint32_t base_ID = G.vertex_read[base_node];
    Entry base{};
    base.m.read = base_ID;
    if (G.vertex_fwd[base_node]) {  // :47-61
        base.m.seq = type == 'l' ? 1 : type == 'r' ? 2 : 0;
        base.m.rev = 0;
    } else {  // :62-76
        base.m.seq = type == 'l' ? 2 : type == 'r' ? 1 : 0;
        base.m.rev = 1;
    }
    base.len = G.len(base_ID, base.m.seq);
    L.seq.push_back(base);
    L.pos.push_back(0);
    L.sorted_vertices.push_back(base_node);
    int64_t total_len = base.len, l_ext = 0, r_ext = 0;
    for (const uint64_t node : vertices) {  // :87
        if (node == base_node) continue;
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
        Entry cur{}, cur1{};
        cur.m.read = current_id;
        cur.m.rev = current_ori ? 0 : 1;
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
                cur1.len = G.len(current_id, cur1.m.seq);
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
        auto insert = [&](const Entry& e, int64_t p) {  // :198-222
            auto it2 = L.pos.begin();
            auto it3 = L.seq.begin();
            auto it5 = L.sorted_vertices.begin();
            for (; it2 != L.pos.end() && *it2 < p; it2++) {
                it3++;
                it5++;
            }
            L.pos.insert(it2, p);
            L.seq.insert(it3, e);
            L.sorted_vertices.insert(it5, node);
        };
        if (current_type == 'p') insert(cur1, new_pos1);
        insert(cur, new_pos);
        int64_t len1, len2;  // :225-240
        if (current_type == 'p') {
            if (new_pos < 0) return HC_SR_EDGE_PAIRED_NEG_POS;  // :227
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
    }
    total_len += l_ext + r_ext;  // :244
    if (total_len > INT32_MAX) return HC_SR_EDGE_BAD_GEOMETRY;
    if (!(total_len > L.pos.back())) return HC_SR_EDGE_BAD_GEOMETRY;  // :246
    const int64_t min = L.pos.front();                                 // :248-252
    if (min < 0)
        for (int64_t& p : L.pos) p -= min;
    if (L.pos.front() != 0 || L.seq.front().len > total_len) return HC_SR_EDGE_BAD_GEOMETRY;  // :256, :259
    int64_t c_pos = 0;
    auto seqit = std::next(L.seq.begin());
    for (auto posit = std::next(L.pos.begin()); posit != L.pos.end(); posit++, seqit++) {  // :261-284
        const int64_t n_pos = *posit;
        if (n_pos < 0 || c_pos > n_pos || n_pos > INT32_MAX || n_pos + seqit->len > total_len) return HC_SR_EDGE_BAD_GEOMETRY;
        c_pos = n_pos;
    }
    L.total_len = total_len;
    return HC_SR_EDGE_OK;
}

typedef std::pair<uint64_t, int> NodeEnd;  // std::pair<node_id_t, int>, :607

// sortVerticesByEndpos (:639-651) with the chosen order among ties
void sort_by_endpos(std::vector<NodeEnd>& pairs, int tie_order) {
    const auto less = [](const NodeEnd& a, const NodeEnd& b) { return a.second < b.second; };
    if (tie_order == 0) {
        std::sort(pairs.begin(), pairs.end(), less);  // :640
        return;
    }
    std::stable_sort(pairs.begin(), pairs.end(), less);
    if (tie_order == 2)
        for (size_t a = 0; a < pairs.size();) {
            size_t b = a;
            while (b < pairs.size() && pairs[b].second == pairs[a].second) b++;
            std::reverse(pairs.begin() + a, pairs.begin() + b);
            a = b;
        }
}

// filter_subreads' selection (:597-622) on (vertex, endpos) in list order.  false: the reference's assert of :619 fires.
bool filter_select(const std::vector<NodeEnd>& in_list_order, uint32_t num, uint64_t base_node, int tie_order, std::set<uint64_t>& selected) {
    selected.clear();
    const size_t left = std::min<size_t>(num / 2, in_list_order.size());
    for (size_t k = 0; k < left; k++) selected.insert(in_list_order[k].first);  // :604
    selected.insert(base_node);                                                  // :605
    std::vector<NodeEnd> pairs = in_list_order;                                  // :607-615
    sort_by_endpos(pairs, tie_order);                                            // :616
    auto last_node = pairs.rbegin();
    while (selected.size() < num) {  // :618-622
        if (last_node == pairs.rend()) return false;
        selected.insert(last_node->first);
        last_node++;
    }
    return true;
}

// The same walk seen per group of equal endpos, by the shared rule: HC_SR_FILTER_GROUPS / _STABLE / _HOST.
uint32_t filter_classify(const std::vector<NodeEnd>& in_list_order, uint32_t num, uint64_t base_node) {
    std::set<uint64_t> selected;
    const size_t left = std::min<size_t>(num / 2, in_list_order.size());
    for (size_t k = 0; k < left; k++) selected.insert(in_list_order[k].first);
    selected.insert(base_node);
    std::vector<NodeEnd> pairs = in_list_order;
    sort_by_endpos(pairs, 1);
    size_t i = pairs.size();
    while (selected.size() < num && i > 0) {
        size_t gs = i;
        while (gs > 0 && pairs[gs - 1].second == pairs[i - 1].second) gs--;
        std::set<uint64_t> fresh;
        for (size_t k = gs; k < i; k++)
            if (!selected.count(pairs[k].first)) fresh.insert(pairs[k].first);
        const GroupStep step = hc::srclique::group_step((uint32_t)fresh.size(), (uint32_t)(num - selected.size()), (uint32_t)pairs.size());
        if (step != hc::srclique::kTakeGroup) return hc::srclique::filter_class(step);
        selected.insert(fresh.begin(), fresh.end());
        i = gs;
    }
    return HC_SR_FILTER_GROUPS;
}

inline void sub_place(int32_t trim, int32_t pos, int32_t& index, int32_t& startpos) {
    if (trim > pos) {
        startpos = trim - pos;
        index = 0;
    } else {
        startpos = 0;
        index = pos - trim;
    }
}

// calcSubreadInfo (:536-595)
std::map<uint64_t, hc_sr_subread_info> calc_subread_info(int32_t trim_pos1, int32_t trim_pos2, const Lists& L1, const Lists& L2) {
    std::map<uint64_t, hc_sr_subread_info> subread_map;
    auto node_it = L1.sorted_vertices.begin();
    for (const int64_t pos : L1.pos) {
        auto it = subread_map.find(*node_it);
        if (it != subread_map.end()) {  // :544-558
            sub_place(trim_pos1, (int32_t)pos, it->second.index2, it->second.startpos2);
        } else {  // :559-572
            hc_sr_subread_info s{-1, -1, -1, -1};
            sub_place(trim_pos1, (int32_t)pos, s.index1, s.startpos1);
            subread_map.insert(std::make_pair(*node_it, s));
        }
        node_it++;
    }
    if (trim_pos2 >= 0) {  // :575-593
        auto node_it2 = L2.sorted_vertices.begin();
        for (const int64_t pos : L2.pos) {
            auto it = subread_map.find(*node_it2);
            if (it != subread_map.end()) sub_place(trim_pos2, (int32_t)pos, it->second.index2, it->second.startpos2);
            node_it2++;
        }
    }
    return subread_map;
}

std::vector<NodeEnd> node_ends(const Lists& L) {  // :607-615
    std::vector<NodeEnd> pairs;
    auto pos_it = L.pos.begin();
    auto seq_it = L.seq.begin();
    for (const uint64_t node : L.sorted_vertices) {
        pairs.push_back(std::make_pair(node, (int)(*pos_it + seq_it->len)));
        pos_it++;
        seq_it++;
    }
    return pairs;
}

}  // namespace

extern "C" {

int hc_host_sr_clique_filter(const uint32_t* vertex, const int32_t* endpos, uint32_t n, uint32_t num, uint32_t base_vertex, int tie_order,
                             uint8_t* used, uint32_t* filter) {
    const char* me = "hc_host_sr_clique_filter: ";
    if (!vertex || !endpos || !used || !filter || n == 0) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "null argument or no entry");
    if (tie_order < 0 || tie_order > 2) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "tie_order is 0, 1 or 2");
    std::vector<NodeEnd> pairs(n);
    bool has_base = false;
    for (uint32_t k = 0; k < n; k++) {
        pairs[k] = std::make_pair((uint64_t)vertex[k], (int)endpos[k]);
        has_base = has_base || vertex[k] == base_vertex;
    }
    if (!has_base) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "the base is no entry of the layout");
    std::set<uint64_t> selected;
    if (!filter_select(pairs, num, base_vertex, tie_order, selected))
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "num exceeds the layout's distinct vertices (assert, src/SRBuilder.cpp:619)");
    for (uint32_t k = 0; k < n; k++) used[k] = selected.count(vertex[k]) ? 1 : 0;  // :626-635
    *filter = filter_classify(pairs, num, base_vertex);
    return HC_OK;
}

int hc_host_sr_clique_merge_layouts(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, const uint64_t* seq_off,
                                    const uint32_t* read_first_seq, uint32_t n_reads, const uint64_t* clique_off, const uint32_t* clique_nodes,
                                    uint64_t n_cliques, const uint32_t* vertex_read, const uint8_t* vertex_fwd, const hc_sr_settings* settings,
                                    uint32_t* clique_status, uint64_t* first_layout, hc_sr_layout* layouts, hc_sr_member* members,
                                    uint32_t* member_vertex, uint8_t* member_used, uint8_t* layout_filter, const int32_t* ret,
                                    hc_sr_subread_info* subreads, hc_sr_clique_stats* stats) {
    const char* me = "hc_host_sr_clique_merge_layouts: ";
    if (stats) memset(stats, 0, sizeof *stats);
    if (!out_off || !seq_off || !read_first_seq || !settings || !first_layout || !clique_off || (n_vertices && (!vertex_read || !vertex_fwd)) ||
        (n_cliques && (!clique_status || !layouts)) || (n_vertices && out_off[n_vertices] && !edges))
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "null argument");
    if (settings->min_clique_size == 0)
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "min_clique_size == 0: filter_subreads (src/SRBuilder.cpp:725) is then called with "
                                                                "num == 0 and may drop the first list entry, a layout the consensus refuses");
    for (uint64_t i = 0; i < n_cliques; i++)
        if (clique_off[i + 1] < clique_off[i]) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "clique_off descends");
    const uint64_t N = clique_off[n_cliques] - clique_off[0];
    if (clique_off[0] != 0) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "clique_off[0] is not 0");
    if (N >= (1ull << 31)) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "2^31 clique entries or more");
    if (N && (!clique_nodes || !members || !member_vertex || !member_used || (ret && !subreads)))
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "null argument");
    const Graph G{edges, out_off, n_vertices, seq_off, read_first_seq, n_reads, vertex_read, vertex_fwd};
    const uint32_t m = settings->min_clique_size;
    uint64_t n_layouts = 0, n_members = 0;
    Lists L1, L2;
    std::set<uint64_t> selected;
    for (uint64_t i = 0; i < n_cliques; i++) {
        first_layout[i] = n_layouts;
        std::vector<uint64_t> clique(clique_nodes + clique_off[i], clique_nodes + clique_off[i + 1]);
        if (subreads)
            for (uint64_t k = clique_off[i]; k < clique_off[i + 1]; k++) subreads[k] = hc_sr_subread_info{-1, -1, -1, -1};
        uint32_t st = HC_SR_EDGE_OK;
        if (clique.size() < 2) st = HC_SR_CLIQUE_TOO_SMALL;  // :656
        std::sort(clique.begin(), clique.end());             // :658
        for (size_t k = 0; k < clique.size() && st == HC_SR_EDGE_OK; k++) {
            if (clique[k] >= n_vertices || vertex_read[clique[k]] >= n_reads) st = HC_SR_EDGE_BAD_VERTEX;
            else if (k && clique[k] == clique[k - 1]) st = clique.size() == 2 ? HC_SR_EDGE_BAD_VERTEX : HC_SR_CLIQUE_REPEATED_VERTEX;
        }
        char superread_type = 'p';
        if (st == HC_SR_EDGE_OK) {
            uint64_t base_node = clique[0];  // :669-679
            for (const uint64_t x : clique)
                if (superread_type == 'p' && !G.paired(vertex_read[x])) {
                    base_node = x;
                    superread_type = 's';
                }
            if (superread_type == 'p') {  // :691-698
                st = sort_vertices(G, clique, 'l', clique[0], L1);
                if (st == HC_SR_EDGE_OK) st = sort_vertices(G, clique, 'r', clique[0], L2);
            } else {
                st = sort_vertices(G, clique, 's', base_node, L1);
                L2.clear();
            }
            if (st == HC_SR_EDGE_OK) {
                const bool filtered = hc::srclique::is_filtered(clique.size(), m);  // :721
                const uint64_t l0 = n_layouts;
                for (int k = 0; k < (superread_type == 'p' ? 2 : 1); k++) {
                    const Lists& L = k ? L2 : L1;
                    uint32_t cls = HC_SR_FILTER_NONE;
                    if (filtered) {  // :725, :728 (base_node is clique[0] for 'p')
                        const std::vector<NodeEnd> pairs = node_ends(L);
                        const uint32_t num = hc::srclique::filter_num(m);
                        if (!filter_select(pairs, num, base_node, 0, selected))
                            return hc::set_last_error(HC_ERR_BAD_OVERLAP, std::string(me) + "filter_subreads ran out of vertices");
                        cls = filter_classify(pairs, num, base_node);
                        if (stats) {
                            stats->n_filtered_layouts++;
                            if (cls == HC_SR_FILTER_HOST) stats->n_host_filters++;
                        }
                    }
                    layouts[n_layouts].first_member = n_members;
                    layouts[n_layouts].n_members = (uint32_t)L.pos.size();
                    layouts[n_layouts].total_len = (int32_t)L.total_len;
                    if (layout_filter) layout_filter[n_layouts] = (uint8_t)cls;
                    auto pos_it = L.pos.begin();
                    auto v_it = L.sorted_vertices.begin();
                    for (const Entry& e : L.seq) {
                        hc_sr_member mm = e.m;
                        mm.pos = (int32_t)*pos_it;
                        members[n_members] = mm;
                        member_vertex[n_members] = (uint32_t)*v_it;
                        member_used[n_members] = !filtered || selected.count(*v_it) ? 1 : 0;  // :626-635
                        n_members++;
                        pos_it++;
                        v_it++;
                    }
                    n_layouts++;
                }
                if (ret && subreads) {  // :748
                    const auto map = calc_subread_info(ret[l0], superread_type == 'p' ? ret[l0 + 1] : -1, L1, L2);
                    for (size_t k = 0; k < clique.size(); k++) {
                        const auto it = map.find(clique[k]);
                        if (it != map.end()) subreads[clique_off[i] + k] = it->second;
                    }
                }
            }
        }
        clique_status[i] = st;
    }
    first_layout[n_cliques] = n_layouts;
    return HC_OK;
}

}  // extern "C"
