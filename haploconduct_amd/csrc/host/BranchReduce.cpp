// BranchReduce.cpp — the second half of BranchReduction::readBasedBranchReduction (reference src/BranchReduction.cpp:82-227, :745-1272) on
// the host: the routines of BranchReduce.h, which hc_br_reduce shares, and around them hc_host_br_reduce (the mirror: the filter of
// :1053-1096 on the lists themselves, OverlapGraph::removeEdge on arrays), hc_host_br_parse_thresholds and hc_host_br_map_order
// (include/hcsr.h).  The reference's containers where their iteration order reaches a result; no device, no context.
#include "BranchReduce.h"

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <unordered_map>
#include <unordered_set>

#include "TargetOrder.h"

namespace hc {
namespace brr {
namespace {

struct Walk {
    std::unordered_map<node_id_t, bool> visited_in_branches, visited_out_branches;
    std::unordered_map<node_id_t, std::list<node_id_t>> branch_in_map, branch_out_map;
    std::unordered_map<node_id_t, int> branch_in_dist_map, branch_out_dist_map;
    std::unordered_set<node_id_t> false_in_branches, false_out_branches;

    void extendComponentIn(std::vector<node_pair_t>& component, const std::list<node_id_t>& neighbors, bool& has_false_branch);

    std::pair<int, node_id_t> extendComponentOut(std::vector<node_pair_t>& component, const std::list<node_id_t>& neighbors, bool& has_false_branch) {  // :941-977
        std::pair<int, node_id_t> dist_node_pair;
        bool extended = false;
        for (auto node : neighbors) {
            auto visited = visited_out_branches.find(node);
            if (visited == visited_out_branches.end() || visited->second == true) continue;
            if (false_out_branches.find(node) != false_out_branches.end()) has_false_branch = true;
            const std::list<node_id_t>& branch = branch_out_map.at(node);
            dist_node_pair = std::make_pair(branch_out_dist_map.at(node), node);
            extended = true;
            for (auto out_neighbor : branch) component.push_back(std::make_pair(node, out_neighbor));
            visited_out_branches.at(node) = true;
            extendComponentIn(component, branch, has_false_branch);
        }
        if (!extended) dist_node_pair = std::make_pair(0, neighbors.front());
        return dist_node_pair;
    }
};

void Walk::extendComponentIn(std::vector<node_pair_t>& component, const std::list<node_id_t>& neighbors, bool& has_false_branch) {  // :979-1007
    for (auto node : neighbors) {
        auto visited = visited_in_branches.find(node);
        if (visited == visited_in_branches.end() || visited->second == true) continue;
        if (false_in_branches.find(node) != false_in_branches.end()) has_false_branch = true;
        const std::list<node_id_t>& branch = branch_in_map.at(node);
        for (auto in_neighbor : branch) component.push_back(std::make_pair(in_neighbor, node));
        visited_in_branches.at(node) = true;
        extendComponentOut(component, branch, has_false_branch);
    }
}

// int arithmetic that wraps where the reference's would overflow
inline int add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
inline int sub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }

}  // namespace

const char* find_components(const hc_br_branch* branches, uint64_t n_branches, const uint32_t* branch_nb, uint64_t n_nb, const Triple* tri, uint64_t V,
                            Components& out) {
    Walk w;
    std::unordered_map<node_id_t, uint64_t> in_row, out_row;  // (not the reference's: where a branch's neighbours and triples lie)
    // :760-781: final_branch_in / final_branch_out are indexed by vertex, so the loops run in ascending vertex, the tables' order
    for (int side = HC_BR_IN; side <= HC_BR_OUT; side++)
        for (uint64_t b = 0; b < n_branches; b++) {
            const hc_br_branch& B = branches[b];
            if (B.side != side || B.nb_count == 0) continue;
            if (B.node >= V || B.nb_first > n_nb || B.nb_count > n_nb - B.nb_first) return "a branch lies outside the graph or outside branch_nb";
            std::list<node_id_t> branch;
            for (uint64_t k = 0; k < B.nb_count; k++) {
                if (branch_nb[B.nb_first + k] >= V || branch_nb[B.nb_first + k] == B.node) return "a branch neighbour is no other vertex of the graph";
                branch.push_back(branch_nb[B.nb_first + k]);
            }
            const node_id_t node = B.node;
            if (side == HC_BR_IN) {
                if (!w.visited_in_branches.insert(std::make_pair(node, false)).second) return "a vertex is listed as an in-branch twice";
                w.branch_in_map.insert(std::make_pair(node, branch));
                w.branch_in_dist_map.insert(std::make_pair(node, (int)B.dist));
                if (B.is_false) w.false_in_branches.insert(node);
                in_row.insert(std::make_pair(node, b));
            } else {
                if (!w.visited_out_branches.insert(std::make_pair(node, false)).second) return "a vertex is listed as an out-branch twice";
                w.branch_out_map.insert(std::make_pair(node, branch));
                w.branch_out_dist_map.insert(std::make_pair(node, (int)B.dist));
                if (B.is_false) w.false_out_branches.insert(node);
                out_row.insert(std::make_pair(node, b));
            }
        }
    auto push = [&](std::vector<node_pair_t>& comp, int dist) {
        hc_br_component c;
        memset(&c, 0, sizeof c);
        c.dist = dist;
        c.min_evidence = -1;
        c.edge_first = out.edges.size();
        c.edge_count = (uint32_t)comp.size();
        std::set<node_id_t> in_nodes, out_nodes;  // :1018-1025, :1045
        for (auto& p : comp) in_nodes.insert(p.second), out_nodes.insert(p.first);
        out.typical.push_back((comp.size() == 3 || comp.size() == 4) && in_nodes.size() == 2 && out_nodes.size() == 2);
        out.edges.insert(out.edges.end(), comp.begin(), comp.end());
        out.comps.push_back(c);
    };
    // :784-863
    for (auto& branch : w.branch_in_map) {
        const node_id_t node = branch.first;
        if (w.visited_in_branches.at(node)) continue;
        const std::list<node_id_t>& neighbors = branch.second;
        std::vector<node_pair_t> new_component;
        bool has_false_branch = w.false_in_branches.find(node) != w.false_in_branches.end();
        for (auto in_neighbor : neighbors) new_component.push_back(std::make_pair(in_neighbor, node));
        w.visited_in_branches.at(node) = true;
        int dist1 = w.branch_in_dist_map.at(node);
        const std::pair<int, node_id_t> dist_node_pair = w.extendComponentOut(new_component, neighbors, has_false_branch);
        int dist2 = dist_node_pair.first;
        const node_id_t outnode = dist_node_pair.second;
        // getEdgeInfo(outnode, node): outnode is one of node's neighbours
        const hc_br_branch& B = branches[in_row.at(node)];
        uint64_t k = 0;
        while (k < B.nb_count && branch_nb[B.nb_first + k] != outnode) k++;
        if (k == B.nb_count) return "the walk returned a vertex that is no neighbour of its branch";
        const Triple& e = tri[B.nb_first + k];
        const int len1 = e.len1, len2 = e.len2, overlap_len = e.olen;
        if (overlap_len < 100) {
            if (dist1 < add(sub(len2, overlap_len), 100)) dist1 = add(sub(len2, overlap_len), 100);
            if (dist2 < add(sub(len1, overlap_len), 100)) dist2 = add(sub(len1, overlap_len), 100);
        } else {
            if (dist1 < len2) dist1 = len2;
            if (dist2 < len1) dist2 = len1;
        }
        const int dist = add(sub(sub(add(dist1, dist2), len1), len2), overlap_len);
        std::sort(new_component.begin(), new_component.end());  // (:837-845: the comparator is the pair's own order)
        new_component.erase(std::unique(new_component.begin(), new_component.end()), new_component.end());
        if (has_false_branch) {
            out.to_remove.insert(out.to_remove.end(), new_component.begin(), new_component.end());
            out.n_false_dropped++;
        } else {
            push(new_component, dist);
        }
    }
    // :882-937
    for (auto& branch : w.branch_out_map) {
        const node_id_t node = branch.first;
        if (w.visited_out_branches.at(node)) continue;
        const std::list<node_id_t>& neighbors = branch.second;
        std::vector<node_pair_t> new_component;
        for (auto out_neighbor : neighbors) new_component.push_back(std::make_pair(node, out_neighbor));
        int dist1 = w.branch_out_dist_map.at(node), dist2;
        const Triple& e = tri[branches[out_row.at(node)].nb_first];  // getEdgeInfo(node, neighbors.front())
        const int len1 = e.len1, len2 = e.len2, overlap_len = e.olen;
        if (overlap_len < 100) {
            if (dist1 < add(sub(len1, overlap_len), 100)) dist1 = add(sub(len1, overlap_len), 100);
            dist2 = add(sub(len2, overlap_len), 100);
        } else {
            if (dist1 < len1) dist1 = len1;
            dist2 = len2;
        }
        const int dist = add(sub(sub(add(dist1, dist2), len1), len2), overlap_len);
        if (w.false_out_branches.find(node) != w.false_out_branches.end()) {
            out.to_remove.insert(out.to_remove.end(), new_component.begin(), new_component.end());
            out.n_false_dropped++;
        } else {
            // (not sorted by the reference, :898-904; the neighbours ascend and do not repeat in hc_br_evidence's tables.  Sorted and
            // de-duplicated here as well, which changes nothing for such tables and keeps comp_edge's contract for any other)
            std::sort(new_component.begin(), new_component.end());
            new_component.erase(std::unique(new_component.begin(), new_component.end()), new_component.end());
            push(new_component, dist);
        }
        w.visited_out_branches.at(node) = true;
    }
    return nullptr;
}

void mark_host_finished(Components& c, bool diploid) {
    std::vector<std::pair<node_pair_t, uint32_t>> all;
    all.reserve(c.edges.size());
    for (uint32_t i = 0; i < c.comps.size(); i++) {
        if (diploid && c.typical[i]) c.comps[i].host_finished |= HC_BR_RED_HOST_DIPLOID;
        for (uint64_t k = 0; k < c.comps[i].edge_count; k++) all.push_back(std::make_pair(c.edges[c.comps[i].edge_first + k], i));
    }
    std::sort(all.begin(), all.end());
    for (size_t k = 1; k < all.size(); k++)
        if (all[k].first == all[k - 1].first) {
            c.comps[all[k].second].host_finished |= HC_BR_RED_HOST_SHARED_EDGE;
            c.comps[all[k - 1].second].host_finished |= HC_BR_RED_HOST_SHARED_EDGE;
        }
}

void look_up_thresholds(const hc_br_reduce_settings* st, const Components& c, std::vector<int32_t>& min_evidence, std::vector<uint8_t>& found) {
    std::map<int, int> evidence_threshold_map;
    for (uint64_t k = 0; k < st->n_thresholds; k++) evidence_threshold_map[st->thresholds[k].dist] = st->thresholds[k].min_evidence;  // :151
    min_evidence.assign(c.comps.size(), -1);
    found.assign(c.comps.size(), 0);
    for (size_t i = 0; i < c.comps.size(); i++) {
        auto p = evidence_threshold_map.find(c.comps[i].dist);
        if (p != evidence_threshold_map.end()) min_evidence[i] = p->second, found[i] = 1;
    }
}

bool decide(const node_pair_t* edges, const uint32_t* count, uint32_t n, uint64_t V, int min_evidence, bool diploid_and_typical, std::vector<node_pair_t>& rm) {
    // unique_evidence_per_edge with the inserts of :1040 (the lists' lengths in place of the lists: the order of a map does not depend on
    // what it maps to)
    std::unordered_map<safe_edge_count_t, unsigned int> unique_evidence_per_edge;
    for (uint32_t k = 0; k < n; k++) unique_evidence_per_edge.insert(std::make_pair((safe_edge_count_t)edges[k].first * V + edges[k].second, count[k]));
    auto evidenceIndexToEdge = [&](safe_edge_count_t index) { return std::make_pair((node_id_t)(index / V), (node_id_t)(index % V)); };
    if (diploid_and_typical) {  // :1098-1236
        std::vector<std::pair<safe_edge_count_t, int>> pairs;
        for (auto& ev : unique_evidence_per_edge) pairs.push_back(std::make_pair(ev.first, (int)ev.second));
        std::sort(pairs.begin(), pairs.end(), [](const std::pair<safe_edge_count_t, int>& a, const std::pair<safe_edge_count_t, int>& b) { return a.second < b.second; });
        std::vector<node_pair_t> supported_edges, unsupported_edges;
        int max_count = 0;
        node_pair_t max_edge(0, 0);
        for (auto& ev_idx : pairs) {
            const node_pair_t node_pair = evidenceIndexToEdge(ev_idx.first);
            const int cnt = (int)unique_evidence_per_edge.at(ev_idx.first);
            if (cnt > max_count) max_count = cnt, max_edge = node_pair;
            (cnt > 0 ? supported_edges : unsupported_edges).push_back(node_pair);
        }
        const bool keep_component = supported_edges.size() > 0;
        auto conflicts = [&](const node_pair_t& p) { return p.first == max_edge.first || p.second == max_edge.second; };
        if (supported_edges.size() == 1) {
            for (auto& p : unsupported_edges)
                if (conflicts(p)) rm.push_back(p);
            return keep_component;
        } else if (supported_edges.size() == 2 && supported_edges.at(0).first != supported_edges.at(1).first &&
                   supported_edges.at(0).second != supported_edges.at(1).second) {
            for (auto& p : unsupported_edges) rm.push_back(p);
            return keep_component;
        } else if (supported_edges.size() == 2) {
            bool keep_complement = false;
            if (pairs.at(0).second - pairs.at(1).second > 0.5 * min_evidence) {  // :1164
                rm.push_back(supported_edges.at(1));
                keep_complement = true;
            }
            for (auto& p : unsupported_edges)
                if (!keep_complement || conflicts(p)) rm.push_back(p);
            return keep_component;
        } else if (supported_edges.size() > 2) {
            int load1 = 0, load2 = 0, i = 0;
            for (auto& p : supported_edges) {  // :1184-1195: pairs.at(i), not the pair of supported edge i
                if (p != max_edge && conflicts(p)) load2 += pairs.at(i).second;
                else load1 += pairs.at(i).second;
                i++;
            }
            if (load1 >= load2) {
                for (auto& p : unsupported_edges)
                    if (p != max_edge && conflicts(p)) rm.push_back(p);
                for (auto& p : supported_edges)
                    if (p != max_edge && conflicts(p)) rm.push_back(p);
            } else {
                for (auto& p : unsupported_edges)
                    if (p == max_edge || (p.first != max_edge.first && p.second != max_edge.second)) rm.push_back(p);
                for (auto& p : supported_edges)
                    if (p == max_edge || (p.first != max_edge.first && p.second != max_edge.second)) rm.push_back(p);
            }
            return keep_component;
        }
    }
    bool keep_component = false;  // :1242-1271
    for (auto& ev : unique_evidence_per_edge) {
        if ((int)ev.second < min_evidence) rm.push_back(evidenceIndexToEdge(ev.first));
        else keep_component = true;
    }
    return keep_component;
}

void run_chain(Components& c, const hc_br_reduce_settings* st, const std::vector<int32_t>& min_evidence, const std::vector<uint8_t>& found,
               const std::function<bool(uint32_t, int, std::vector<node_pair_t>&)>& count_component) {
    const size_t n = c.comps.size();
    // :93-127: the components a component shares a vertex with (itself included)
    std::vector<std::set<unsigned int>> neighboring_components(n);
    if (st->careful) {
        std::map<node_id_t, std::set<unsigned int>> nodes_to_components;  // (only the vertices in use: at() of any other is never called)
        for (unsigned int idx = 0; idx < n; idx++)
            for (uint64_t k = 0; k < c.comps[idx].edge_count; k++) {
                const node_pair_t& p = c.edges[c.comps[idx].edge_first + k];
                nodes_to_components[p.first].emplace(idx);
                nodes_to_components[p.second].emplace(idx);
            }
        for (unsigned int idx = 0; idx < n; idx++)
            for (uint64_t k = 0; k < c.comps[idx].edge_count; k++) {
                const node_pair_t& p = c.edges[c.comps[idx].edge_first + k];
                const std::set<unsigned int>&s1 = nodes_to_components.at(p.first), &s2 = nodes_to_components.at(p.second);
                neighboring_components[idx].insert(s1.begin(), s1.end());
                neighboring_components[idx].insert(s2.begin(), s2.end());
            }
    }
    std::set<unsigned int> components_kept;
    for (unsigned int idx = 0; idx < n; idx++) {  // :163-204
        hc_br_component& C = c.comps[idx];
        const node_pair_t* component = c.edges.data() + C.edge_first;
        bool skip = false;
        for (auto comp_idx : neighboring_components[idx]) {
            if (comp_idx == idx) continue;
            if (components_kept.find(comp_idx) != components_kept.end()) {
                c.to_remove.insert(c.to_remove.end(), component, component + C.edge_count);
                skip = true;
            }
        }
        if (skip) {
            C.outcome = HC_BR_RED_CAREFUL;
            C.min_evidence = -1;
            continue;
        }
        C.min_evidence = found[idx] ? min_evidence[idx] : -1;
        if (!found[idx]) {
            c.to_remove.insert(c.to_remove.end(), component, component + C.edge_count);
            C.outcome = HC_BR_RED_NO_THRESHOLD;
            continue;
        }
        const bool keep = count_component(idx, min_evidence[idx], c.to_remove);
        if (keep) components_kept.insert(idx);
        C.outcome = keep ? HC_BR_RED_KEPT : HC_BR_RED_NOT_KEPT;
    }
}

void finish_removals(Components& c) {
    std::sort(c.to_remove.begin(), c.to_remove.end());
    c.to_remove.erase(std::unique(c.to_remove.begin(), c.to_remove.end()), c.to_remove.end());
}

int64_t Evidence::row_of(node_id_t u, node_id_t v) const {
    uint64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint64_t a = ev_edge[2 * mid], b = ev_edge[2 * mid + 1];
        if (a < u || (a == u && b < v)) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_rows && ev_edge[2 * lo] == u && ev_edge[2 * lo + 1] == v ? (int64_t)lo : -1;
}

void count_unique(Evidence& ev, const node_pair_t* edges, uint32_t n, uint32_t* count, bool* no_row) {
    std::vector<int64_t> row(n);           // index_to_mapID, as rows of the tables (-1: evidence_per_edge.at() would throw)
    std::vector<bool> evidence_status;
    for (uint32_t idx = 0; idx < n; idx++) {  // :1022-1042
        row[idx] = ev.row_of(edges[idx].first, edges[idx].second);
        count[idx] = 0;
        if (row[idx] < 0) *no_row = true;                                                              // :1029-1031: nothing is pushed
        else evidence_status.push_back(ev.front[row[idx]] < ev.ev_off[row[idx] + 1]);
    }
    const unsigned int component_edge_count = (unsigned int)evidence_status.size();
    if (evidence_status.empty()) throw std::string("max_element of an empty evidence_status (:1053): no edge of a component has a key in evidence_per_edge");
    auto list_of = [&](unsigned int idx) -> int64_t {
        if (row[idx] < 0) throw std::string("evidence_per_edge.at() of a key it does not hold (:1059, behind :1029-1031)");
        if (ev.front[row[idx]] >= ev.ev_off[row[idx] + 1]) throw std::string("front() of an empty evidence list (:1060, behind :1029-1031)");
        return row[idx];
    };
    while (*std::max_element(evidence_status.begin(), evidence_status.end()) == 1) {  // :1053-1096
        // the minimum over the fronts and whether exactly one list has it (the sorted current_evidence's first two entries)
        bool any = false, unique_min = true;
        uint32_t current_min = 0;
        for (unsigned int idx = 0; idx < component_edge_count; idx++)
            if (evidence_status.at(idx) == 1) {
                const uint32_t f = ev.ev_ids[ev.front[list_of(idx)]];
                if (!any || f < current_min) current_min = f, unique_min = true, any = true;
                else if (f == current_min) unique_min = false;
            }
        for (unsigned int idx = 0; idx < component_edge_count; idx++)
            if (evidence_status.at(idx) == 1) {
                // (two indices may name one row only behind :1029-1031, where an earlier index has popped the list empty: the reference's
                // front() of that copy is then front() of an empty list)
                const int64_t r = list_of(idx);
                if (ev.ev_ids[ev.front[r]] == current_min) {
                    if (unique_min) count[idx]++;  // unique_evidence_per_edge.at(mapID).push_back: mapID is edge idx's
                    const bool last = ev.ev_off[r + 1] - ev.front[r] == 1;
                    ev.front[r]++;
                    if (last) evidence_status.at(idx) = 0;
                }
            }
    }
}

void fill_counts(const Components& c, hc_br_reduce_counts* counts) {
    counts->n_components = c.comps.size();
    counts->n_component_edges = c.edges.size();
    counts->n_false_dropped = c.n_false_dropped;
    counts->n_removed = c.to_remove.size();
    for (auto& C : c.comps) {
        counts->n_no_threshold += C.outcome == HC_BR_RED_NO_THRESHOLD;
        counts->n_careful_dropped += C.outcome == HC_BR_RED_CAREFUL;
        counts->n_kept += C.outcome == HC_BR_RED_KEPT;
        counts->n_host_finished += C.host_finished != 0;
    }
}

}  // namespace brr
}  // namespace hc

namespace {

using namespace hc::brr;

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

// std::stoi(tmp) as :147 / :150 call it: true and the value, or false where it throws
bool stoi_like(const std::string& s, int* out) {
    const char* p = s.c_str();
    char* end = nullptr;
    errno = 0;
    const long v = strtol(p, &end, 10);
    if (end == p || errno == ERANGE || v < INT_MIN || v > INT_MAX) return false;
    *out = (int)v;
    return true;
}

}  // namespace

extern "C" {

int hc_host_br_parse_thresholds(const char* text, uint64_t len, hc_br_threshold* out, uint64_t cap, uint64_t* n, uint64_t* bad_line) {
    const char* me = "hc_host_br_parse_thresholds";
    if (!n || (len && !text)) return fail(me, HC_ERR_ARG, "null argument");
    *n = 0;
    if (bad_line) *bad_line = 0;
    std::map<int, int> evidence_threshold_map;
    // the reference's one stringstream: `ss << line` appends, three getline(ss, tmp, '\t') read, ss.clear() resets the flags and leaves
    // what was not read — a fourth field stays in front of the next line
    std::string ss, tmp;
    size_t rd = 0;
    bool eofbit = false, failbit = false;
    auto getline_tab = [&]() {
        if (eofbit || failbit) {  // the sentry fails: tmp stays as it is
            failbit = true;
            return;
        }
        tmp.erase();
        bool delim = false;
        while (rd < ss.size()) {
            const char ch = ss[rd++];
            if (ch == '\t') {
                delim = true;
                break;
            }
            tmp.push_back(ch);
        }
        if (!delim) {
            eofbit = true;
            if (tmp.empty()) failbit = true;
        }
    };
    uint64_t at = 0, line_no = 0;
    while (at < len) {  // getline(thresholds_file, line): the last line needs no '\n'
        const char* nl = (const char*)memchr(text + at, '\n', len - at);
        const uint64_t end = nl ? (uint64_t)(nl - text) : len;
        const std::string line(text + at, end - at);
        at = end + 1;
        line_no++;
        if (line.empty() || line.front() == '#') continue;
        ss.erase(0, rd), rd = 0;
        ss += line;
        int dist = 0, min_ev = 0;
        getline_tab();
        bool ok = stoi_like(tmp, &dist);
        getline_tab();
        getline_tab();
        ok = ok && stoi_like(tmp, &min_ev);
        if (!ok) {
            if (bad_line) *bad_line = line_no;
            return fail(me, HC_ERR_ARG, "std::stoi throws on line " + std::to_string(line_no));
        }
        evidence_threshold_map[dist] = min_ev;
        eofbit = failbit = false;  // ss.clear()
    }
    *n = evidence_threshold_map.size();
    if (*n && (!out || cap < *n)) return fail(me, HC_ERR_ARG, "room for fewer entries than the table has");
    uint64_t k = 0;
    for (auto& e : evidence_threshold_map) out[k].dist = e.first, out[k].min_evidence = e.second, k++;
    return HC_OK;
}

int hc_host_br_map_order(uint64_t n, uint64_t* order) {
    if (n && !order) return fail("hc_host_br_map_order", HC_ERR_ARG, "null argument");
    std::unordered_map<node_id_t, bool> m;
    for (uint64_t k = 0; k < n; k++) m.insert(std::make_pair((node_id_t)k, false));
    uint64_t k = 0;
    for (auto& e : m) order[k++] = e.first;
    return HC_OK;
}

int hc_host_br_reduce(const hc_br_host_input* in, const hc_br_tables* ev, const hc_br_reduce_settings* st, hc_br_reduce_counts* counts, hc_br_reduce_tables* T,
                      hc_br_host_graph_out* G) {
    const char* me = "hc_host_br_reduce";
    if (!in || !ev || !st || !counts) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    if (G) G->n_edges = G->n_branching = 0;
    if (!st->n_thresholds || !st->thresholds) return fail(me, HC_ERR_ARG, "an empty threshold table (the exit(1) of :157)");
    const uint64_t V = in->n_vertices;
    if (!in->out_off || !in->in_off) return fail(me, HC_ERR_ARG, "null offsets");
    const uint64_t E = in->out_off[V];
    if (in->in_off[V] != E || (E && (!in->edges || !in->in_nodes))) return fail(me, HC_ERR_ARG, "adj_in and adj_out differ in size, or a null array");
    const uint64_t n_b = ev->cap_branches, n_nb = ev->cap_branch_nb, n_rows = ev->cap_ev_edges, n_missing = ev->cap_missing;
    if ((n_b && !ev->branches) || (n_nb && !ev->branch_nb) || (n_rows && (!ev->ev_edge || !ev->ev_off)) || (ev->cap_ev_ids && !ev->ev_ids) ||
        (n_missing && !ev->missing_edges))
        return fail(me, HC_ERR_ARG, "a null table");
    if (n_rows && ev->ev_off[n_rows] > ev->cap_ev_ids) return fail(me, HC_ERR_ARG, "ev_off names more ids than ev_ids holds");
    // sortAdjOut (:48): position -> record
    std::vector<uint32_t> order(E);
    {
        std::vector<uint32_t> targets, perm;
        for (uint64_t v = 0; v < V; v++) {
            const uint64_t a = in->out_off[v], n = in->out_off[v + 1] - a;
            targets.resize(n), perm.resize(n);
            for (uint64_t k = 0; k < n; k++) targets[k] = (uint32_t)in->edges[a + k].v2;
            hc::target_sort_perm(targets.data(), n, perm.data());
            for (uint64_t k = 0; k < n; k++) order[a + k] = (uint32_t)(a + perm[k]);
        }
    }
    auto first_record = [&](uint64_t u, uint64_t v) -> int64_t {  // getEdgeInfo / checkEdge / removeEdge: the first u -> v in list order
        if (u >= V) return -1;
        for (uint64_t k = in->out_off[u]; k < in->out_off[u + 1]; k++)
            if (in->edges[order[k]].v2 == v) return (int64_t)k;
        return -1;
    };
    auto read_len = [&](uint64_t r, int32_t* len) {  // Read::get_len()
        if (r >= in->n_reads) return false;
        const uint32_t f = in->read_first_seq[r], l = in->read_first_seq[r + 1];
        *len = (int32_t)(uint32_t)(in->seq_off[l] - in->seq_off[f]);
        return true;
    };
    // the records the walk asks getEdgeInfo for
    std::vector<Triple> tri(n_nb ? n_nb : 1);
    for (uint64_t b = 0; b < n_b; b++) {
        const hc_br_branch& B = ev->branches[b];
        if (B.nb_first > n_nb || B.nb_count > n_nb - B.nb_first) return fail(me, HC_ERR_ARG, "a branch lies outside branch_nb");
        for (uint64_t k = 0; k < B.nb_count; k++) {
            const uint64_t x = ev->branch_nb[B.nb_first + k];
            const int64_t p = B.side == HC_BR_OUT ? first_record(B.node, x) : first_record(x, B.node);
            if (p < 0) return fail(me, HC_ERR_ARG, "a branch neighbour without a record in the graph (getEdgeInfo exits)");
            const hc_edge_rec& e = in->edges[order[p]];
            Triple& t = tri[B.nb_first + k];
            t.olen = e.len0;
            if (!read_len(e.read1, &t.len1) || !read_len(e.read2, &t.len2)) return fail(me, HC_ERR_ARG, "a record's read is no read of the store");
        }
    }
    Components c;
    if (const char* what = find_components(ev->branches, n_b, ev->branch_nb, n_nb, tri.data(), V, c)) return fail(me, HC_ERR_ARG, what);
    mark_host_finished(c, st->diploid != 0);
    std::vector<int32_t> min_evidence;
    std::vector<uint8_t> found;
    look_up_thresholds(st, c, min_evidence, found);
    Evidence lists(ev->ev_edge, ev->ev_off, ev->ev_ids, n_rows);
    std::vector<uint32_t> unique(c.edges.size() ? c.edges.size() : 1, 0);
    try {
        run_chain(c, st, min_evidence, found, [&](uint32_t i, int min_ev, std::vector<node_pair_t>& rm) {
            hc_br_component& C = c.comps[i];
            bool no_row = false;
            count_unique(lists, c.edges.data() + C.edge_first, C.edge_count, unique.data() + C.edge_first, &no_row);
            if (no_row) C.host_finished |= HC_BR_RED_HOST_NO_ROW;
            return decide(c.edges.data() + C.edge_first, unique.data() + C.edge_first, C.edge_count, V, min_ev, st->diploid && c.typical[i], rm);
        });
    } catch (const std::string& what) {
        return fail(me, HC_ERR_ARG, what);
    }
    // (a component the chain skipped is never looked up: the bit of :1029 is set for it as the device call sets it, from the tables)
    for (size_t i = 0; i < c.comps.size(); i++)
        for (uint64_t k = 0; k < c.comps[i].edge_count; k++)
            if (lists.row_of(c.edges[c.comps[i].edge_first + k].first, c.edges[c.comps[i].edge_first + k].second) < 0) c.comps[i].host_finished |= HC_BR_RED_HOST_NO_ROW;
    finish_removals(c);
    fill_counts(c, counts);
    counts->n_missing_appended = n_missing;
    for (auto& C : c.comps)
        for (uint64_t k = 0; k < C.edge_count; k++) {
            const int64_t r = lists.row_of(c.edges[C.edge_first + k].first, c.edges[C.edge_first + k].second);
            if (r >= 0) counts->n_items_sorted += ev->ev_off[r + 1] - ev->ev_off[r];
        }
    // :217-225 on a copy's marks: every pair has a record, or nothing is written
    std::vector<uint8_t> gone(E ? E : 1, 0), in_gone(E ? E : 1, 0);
    std::vector<uint64_t> removed_at;
    for (auto& p : c.to_remove) {
        const int64_t k = first_record(p.first, p.second);
        if (k < 0) return fail(me, HC_ERR_ARG, "a pair of edges_to_remove has no record in the graph (the exit(1) of :219-222)");
        gone[k] = 1;  // (positions of the SORTED list; a pair is listed once, so its twins stay)
        removed_at.push_back((uint64_t)k);
        uint64_t q = in->in_off[p.second];
        while (q < in->in_off[p.second + 1] && (in->in_nodes[q] != p.first || in_gone[q])) q++;
        if (q < in->in_off[p.second + 1]) in_gone[q] = 1;  // (removeEdge does not insist on the adj_in entry, :132-145)
    }
    const uint64_t n_left = E - removed_at.size();
    if (G) {
        G->n_edges = n_left;
        G->n_branching = n_missing + removed_at.size();
    }
    int rc = HC_OK;
    if (T) {
        if ((T->components && T->cap_components < c.comps.size()) || ((T->comp_edge || T->comp_unique) && T->cap_comp_edges < c.edges.size()) ||
            (T->removed && T->cap_removed < c.to_remove.size()))
            rc = fail(me, HC_ERR_ARG, "a table is too small (the counts say how large)");
        else {
            if (T->components && !c.comps.empty()) memcpy(T->components, c.comps.data(), c.comps.size() * sizeof(hc_br_component));
            for (size_t k = 0; k < c.edges.size(); k++) {
                if (T->comp_edge) T->comp_edge[2 * k] = (uint32_t)c.edges[k].first, T->comp_edge[2 * k + 1] = (uint32_t)c.edges[k].second;
                if (T->comp_unique) T->comp_unique[k] = unique[k];
            }
            if (T->removed)
                for (size_t k = 0; k < c.to_remove.size(); k++)
                    T->removed[2 * k] = (uint32_t)c.to_remove[k].first, T->removed[2 * k + 1] = (uint32_t)c.to_remove[k].second;
        }
    }
    if (G && (G->edges || G->out_off || G->in_nodes || G->in_off || G->branching)) {
        if ((G->edges && G->cap_edges < n_left) || (G->in_nodes && G->cap_edges < n_left) || (G->branching && G->cap_branching < G->n_branching))
            return fail(me, HC_ERR_ARG, "the graph's arrays are too small (n_edges / n_branching say how large)");
        uint64_t w = 0, wi = 0;
        for (uint64_t v = 0; v < V; v++) {
            if (G->out_off) G->out_off[v] = w;
            if (G->in_off) G->in_off[v] = wi;
            for (uint64_t k = in->out_off[v]; k < in->out_off[v + 1]; k++)
                if (!gone[k]) {
                    if (G->edges) G->edges[w] = in->edges[order[k]];
                    w++;
                }
            for (uint64_t q = in->in_off[v]; q < in->in_off[v + 1]; q++)
                if (!in_gone[q]) {
                    if (G->in_nodes) G->in_nodes[wi] = in->in_nodes[q];
                    wi++;
                }
        }
        if (G->out_off) G->out_off[V] = w;
        if (G->in_off) G->in_off[V] = wi;
        if (G->branching) {
            for (uint64_t k = 0; k < n_missing; k++) G->branching[k] = ev->missing_edges[k];
            for (size_t k = 0; k < removed_at.size(); k++) G->branching[n_missing + k] = in->edges[order[removed_at[k]]];
        }
    }
    return rc;
}

}  // extern "C"
