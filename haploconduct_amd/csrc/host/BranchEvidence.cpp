// BranchEvidence.cpp — hc_host_br_evidence (include/hcsr.h): the host mirror of hc_br_evidence.  BranchReduction::findBranchingEvidence with
// buildDiffListOut, buildDiffListIn, findDiffPos and checkReadEvidence (reference src/BranchReduction.cpp:229-743) and the caller's two loops
// (:60-80), loop by loop on the arrays hc_graph_fetch, the store loader and hc_sr_originals_fetch use.  Strings and lists where the
// reference has them; an unordered_map over a read's originals is a binary search here (the dict's entries are in ascending id), and
// evidence_per_edge is a std::map over (u, v), which is the order the tables list it in.  No device, no context.
#include "BranchEvidence.h"

#include <algorithm>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "TargetOrder.h"

namespace hc {
namespace br {

const char* check_settings(const hc_br_settings* st, uint64_t n_original_reads) {
    if (st->original_readcount >= (1ull << 31)) return "original_readcount is 2^31 or more";
    if (st->se_count > n_original_reads || st->pe_count > n_original_reads || st->se_count + 2 * st->pe_count != n_original_reads)
        return "se_count + 2 * pe_count is not the number of original reads";
    return nullptr;
}

const char* check_original_reads(const uint8_t* bases, const uint64_t* seq_off, uint64_t n_reads) {
    if (!seq_off) return "null offsets";
    if (n_reads >= (1ull << 32)) return "2^32 original reads or more";
    if (seq_off[0] != 0) return "the offsets do not start at 0";
    for (uint64_t r = 0; r < n_reads; r++)
        if (seq_off[r + 1] < seq_off[r]) return "the offsets descend";
    if (seq_off[n_reads] && !bases) return "null bases";
    return nullptr;
}

}  // namespace br
}  // namespace hc

namespace {

using hc::br::complement;

int fail(int status, const std::string& what) { return hc::set_last_error(status, "hc_host_br_evidence: " + what); }

struct View {
    const hc_br_host_input* in;
    const hc_br_settings* st;
    std::vector<uint32_t> order;     // sorted adj_out: position -> record of in->edges (sortAdjOut, :48)
    std::vector<uint32_t> sorted_in; // sortAdjLists(adj_in), :47
};

// the outcome of one findBranchingEvidence call
struct Branch {
    uint32_t node = 0;
    bool outbranch = false;
    uint32_t n_neighbours = 0;
    uint8_t status = HC_BR_OK;
    bool is_false = false, arg_error = false;
    int dist = 0;
    std::list<uint32_t> final_branch;  // without its front entry
    std::list<int> diff_list;
    std::vector<hc_edge_rec> missing_edges;
    std::vector<std::pair<uint32_t, std::list<uint32_t>>> stored;  // the (neighbour, evidence) pairs :350-391 stores, in order
    uint64_t n_items = 0;
};

// getEdgeInfo(v, w, false), src/OverlapGraph.cpp:263-282: the first record v -> w in list order; nullptr where the reference exits
const hc_edge_rec* edge_info(const View& g, uint64_t v, uint64_t w) {
    for (uint64_t k = g.in->out_off[v]; k < g.in->out_off[v + 1]; k++) {
        const hc_edge_rec* e = g.in->edges + g.order[k];
        if (e->v2 == w) return e;
    }
    return nullptr;
}

struct StoreRead {
    bool ok = false, paired = false;
    std::string seq1;      // get_seq(0) of a single-end read
    unsigned int len = 0;  // Read::get_len()
};

StoreRead store_read(const View& g, uint64_t r, bool want_seq) {
    StoreRead x;
    if (r >= g.in->n_reads) return x;
    const uint32_t first = g.in->read_first_seq[r], n = g.in->read_first_seq[r + 1] - first;
    x.ok = true;
    x.paired = n == 2;
    const uint64_t a = g.in->seq_off[first], b = g.in->seq_off[first + 1];
    x.len = (unsigned int)(b - a);
    if (x.paired) x.len += (unsigned int)(g.in->seq_off[first + 2] - b);
    if (want_seq && !x.paired) x.seq1.assign((const char*)g.in->bases + a, b - a);
    return x;
}

std::string build_rev_comp(const std::string& seq) {  // src/Types.h:109-129
    std::string out;
    out.reserve(seq.size());
    for (auto it = seq.rbegin(); it != seq.rend(); it++) out.push_back((char)complement((uint8_t)*it));
    return out;
}

std::vector<int> findDiffPos(const std::string& seq1, const std::string& seq2) {  // :693-713
    std::vector<int> diff_pos;
    int pos = 0;
    auto it1 = seq1.begin(), it2 = seq2.begin();
    while (it1 != seq1.end()) {
        if (*it1 != *it2) {
            diff_pos.push_back(pos);
            if (diff_pos.size() == HC_BR_MAX_DIFFS) return diff_pos;
        }
        it1++, it2++, pos++;
    }
    return diff_pos;
}

bool checkReadEvidence(const std::string& contig, int startpos, const std::string& read, int index, const std::list<int>& diff_list) {  // :716-743
    bool true_evidence = false;
    const int read_start = startpos + index;
    const int read_end = hc::br::int_plus_size(read_start, read.size());
    const int contig_start = startpos;
    const int contig_end = hc::br::int_plus_size(startpos, contig.size());
    for (int diff_pos : diff_list) {
        if (diff_pos < read_start || diff_pos >= read_end) continue;
        else if (diff_pos < contig_start || diff_pos >= contig_end) continue;
        if (read.at(diff_pos - read_start) != contig.at(diff_pos - contig_start)) {
            true_evidence = false;
            break;
        } else {
            true_evidence = true;
        }
    }
    return true_evidence;
}

hc_edge_rec missing_edge(const View& g, int relative_pos, int len, uint64_t min_size, const hc_edge_rec* first, const hc_edge_rec* second, uint32_t v1,
                         uint32_t v2, bool outbranch) {  // :476-511, :630-665
    hc_edge_rec e;
    memset(&e, 0, sizeof e);
    e.score = g.st->edge_threshold;
    e.mismatch_rate = -1;
    e.pos1 = relative_pos;
    e.ori1 = outbranch ? first->ori2 : first->ori1;
    e.ori2 = outbranch ? second->ori2 : second->ori1;
    e.ord = '-';
    e.read1 = outbranch ? first->read2 : first->read1;
    e.read2 = outbranch ? second->read2 : second->read1;
    e.v1 = v1, e.v2 = v2;
    e.perc = hc::br::overlap_perc(len, min_size);
    e.len0 = e.len1 = len;
    return e;
}

// buildDiffListOut (:396-535) / buildDiffListIn (:537-689).  false: an assert of the reference failed (B.status says which).
bool build_diff_list(const View& g, Branch& B, const std::vector<uint32_t>& neighbors, std::vector<std::string>& sequence_vec,
                     std::vector<int>& startpos_vec, std::vector<std::pair<uint32_t, uint32_t>>& missing_inclusion_edges) {
    const uint32_t node1 = B.node;
    const bool outbranch = B.outbranch, fwd = g.in->vertex_fwd[node1] != 0;
    const unsigned int min_overlap_len = g.st->min_overlap_len;
    std::vector<const hc_edge_rec*> edge_vec;
    std::vector<int> pos_vec;
    int node1_len = 0;
    // what the device call refuses with HC_ERR_ARG, for every neighbour and ahead of any assert: a record that is not there, a read of it
    // (read2 of an out-branch's record, read1 and read2 of an in-branch's) that is no read of the store
    for (uint32_t node : neighbors) {
        const hc_edge_rec* edge = outbranch ? edge_info(g, node1, node) : edge_info(g, node, node1);
        if (!edge || edge->read2 >= g.in->n_reads || (!outbranch && edge->read1 >= g.in->n_reads)) return B.arg_error = true, false;
    }
    for (uint32_t node : neighbors) {
        const hc_edge_rec* edge = outbranch ? edge_info(g, node1, node) : edge_info(g, node, node1);
        const StoreRead read = store_read(g, outbranch ? edge->read2 : edge->read1, true);
        if (!read.ok) return B.arg_error = true, false;
        if (read.paired) return B.status = HC_BR_PAIRED_NEIGHBOUR, false;  // :412, :554
        sequence_vec.push_back(fwd ? read.seq1 : build_rev_comp(read.seq1));  // node1's orientation, :414, :556
        pos_vec.push_back(edge->pos1);
        edge_vec.push_back(edge);
        if (!outbranch && node1_len == 0) {
            const StoreRead r2 = store_read(g, edge->read2, false);
            if (!r2.ok) return B.arg_error = true, false;
            node1_len = (int)r2.len;
        }
    }
    if (outbranch) {
        startpos_vec = pos_vec;
    } else {
        const int max_pos = *std::max_element(pos_vec.begin(), pos_vec.end());
        for (int pos : pos_vec) startpos_vec.push_back(max_pos - pos);
    }
    std::vector<int> distance_vec;
    for (unsigned int i = 0; i < neighbors.size(); i++) {
        for (unsigned int j = i + 1; j < neighbors.size(); j++) {
            const uint32_t node_i = neighbors[i], node_j = neighbors[j];
            const std::string &seq_i = sequence_vec[i], &seq_j = sequence_vec[j];
            const int pos_i = startpos_vec[i], pos_j = startpos_vec[j];
            if (node_i == node_j) return B.status = HC_BR_REPEATED_NEIGHBOUR, false;  // :446
            int relative_pos, len, startpos;
            std::string subseq_i, subseq_j;
            if (pos_i < pos_j) {
                relative_pos = pos_j - pos_i;
                if (relative_pos > hc::br::size_minus_min_overlap(seq_i.size(), min_overlap_len)) {
                    if (!outbranch) return B.status = HC_BR_BAD_GEOMETRY, false;  // :605
                    missing_inclusion_edges.push_back(std::make_pair(node_i, node_j));
                    continue;
                }
                if ((uint64_t)relative_pos > seq_i.size()) return B.status = HC_BR_BAD_GEOMETRY, false;  // substr throws
                len = (int)std::min(seq_i.size() - relative_pos, seq_j.size());
                subseq_i = seq_i.substr(relative_pos, len);
                subseq_j = seq_j.substr(0, len);
                startpos = pos_j;
            } else {
                relative_pos = pos_i - pos_j;
                if (relative_pos > hc::br::size_minus_min_overlap(seq_j.size(), min_overlap_len)) {
                    if (!outbranch) return B.status = HC_BR_BAD_GEOMETRY, false;  // :616
                    missing_inclusion_edges.push_back(std::make_pair(node_j, node_i));
                    continue;
                }
                if ((uint64_t)relative_pos > seq_j.size()) return B.status = HC_BR_BAD_GEOMETRY, false;
                len = (int)std::min(seq_j.size() - relative_pos, seq_i.size());
                subseq_i = seq_i.substr(0, len);
                subseq_j = seq_j.substr(relative_pos, len);
                startpos = pos_i;
            }
            if (!outbranch) {
                std::reverse(subseq_i.begin(), subseq_i.end());
                std::reverse(subseq_j.begin(), subseq_j.end());
            }
            const std::vector<int> diff_pos = findDiffPos(subseq_i, subseq_j);
            if (!(len > 0)) return B.status = HC_BR_BAD_GEOMETRY, false;  // :471, :625
            for (int pos : diff_pos) B.diff_list.push_back(outbranch ? pos + startpos : len - pos + startpos);  // :473, :627
            if (diff_pos.empty()) {
                const bool i_first = pos_i < pos_j || (pos_i == pos_j && node_i < node_j);
                const unsigned a = i_first ? i : j, b = i_first ? j : i;
                B.missing_edges.push_back(missing_edge(g, relative_pos, len, std::min(seq_i.size(), seq_j.size()), edge_vec[a], edge_vec[b], neighbors[a],
                                                       neighbors[b], outbranch));
                B.is_false = true;
            } else if (i == 0) {
                if (outbranch) {
                    distance_vec.push_back(diff_pos.at(0) + startpos);
                } else {
                    const int overlap_len = (int)(uint32_t)std::min(seq_i.size() - (size_t)pos_vec[i], seq_j.size() - (size_t)pos_vec[j]);  // :600-602
                    distance_vec.push_back((int)((uint32_t)diff_pos.at(0) + (uint32_t)node1_len - (uint32_t)overlap_len));       // :670
                }
            }
        }
    }
    B.dist = 0;
    if (!distance_vec.empty())
        B.dist = 0.5 * (*std::min_element(distance_vec.begin(), distance_vec.end()) + *std::max_element(distance_vec.begin(), distance_vec.end()));
    B.diff_list.sort();
    B.diff_list.unique();
    return true;
}

// findBranchingEvidence, :229-394, up to where it touches evidence_per_edge: B.stored is what it would store, in order
void find_branching_evidence(const View& g, Branch& B, const std::vector<uint32_t>& neighbors) {
    const hc_br_host_input& in = *g.in;
    const uint32_t node1 = B.node;
    std::list<uint32_t> final_branch(neighbors.begin(), neighbors.end());
    final_branch.push_front(node1);
    std::vector<std::string> sequence_vec;
    std::vector<int> startpos_vec;
    std::vector<std::pair<uint32_t, uint32_t>> missing_inclusion_edges;
    if (!build_diff_list(g, B, neighbors, sequence_vec, startpos_vec, missing_inclusion_edges)) return;
    const uint64_t SE_count = g.st->se_count, PE_count = g.st->pe_count, original_readcount = g.st->original_readcount;
    const uint32_t r1 = in.vertex_read[node1];
    const hc_sr_original *s1 = in.entries + in.orig_off[r1], *s1_end = in.entries + in.orig_off[r1 + 1];
    auto in_subreads1 = [&](uint64_t id) {
        const hc_sr_original* f = std::lower_bound(s1, s1_end, id, [](const hc_sr_original& e, uint64_t x) { return e.id < x; });
        return f != s1_end && f->id == id;
    };
    std::map<uint32_t, std::list<uint32_t>> evidence_per_neighbor;
    for (size_t n = 0; n < neighbors.size(); n++) {
        const uint32_t node2 = neighbors[n], r2 = in.vertex_read[node2];
        std::list<uint32_t> evidence_list;
        const std::string& contig = sequence_vec[n];
        const int startpos = startpos_vec[n];
        for (uint64_t k = in.orig_off[r2]; k < in.orig_off[r2 + 1]; k++) {
            const hc_sr_original& subread = in.entries[k];
            B.n_items++;
            const uint64_t subread_id = subread.id;
            const bool common_subread = in_subreads1(subread_id);
            uint64_t subread_id_PE = 0;
            const bool common_PE = hc::br::mate_of(subread_id, SE_count, PE_count, &subread_id_PE) && in_subreads1(subread_id_PE);
            if (!common_subread && !common_PE) continue;
            if (subread_id >= in.n_original_reads) {  // get_read, :288 / :306
                B.status = HC_BR_BAD_ORIGINAL;
                continue;
            }
            const uint64_t a = in.original_seq_off[subread_id], b = in.original_seq_off[subread_id + 1];
            std::string sequence((const char*)in.original_bases + a, b - a);
            if (!subread.forward) sequence = build_rev_comp(sequence);
            const bool result = checkReadEvidence(contig, startpos, sequence, subread.index1, B.diff_list);  // result1 and result2 are one check
            if (common_subread && result) {
                if (!(subread_id < 2 * original_readcount)) B.status = HC_BR_BAD_ORIGINAL;  // :300
                else evidence_list.push_back((uint32_t)subread_id);
            }
            if (common_PE && result) {
                const uint64_t joint_id = original_readcount + std::min(subread_id, subread_id_PE);
                if (!(joint_id < 2 * original_readcount)) B.status = HC_BR_BAD_ORIGINAL;  // :319
                else evidence_list.push_back((uint32_t)joint_id);
            }
        }
        evidence_list.sort();
        evidence_list.unique();
        evidence_per_neighbor.insert(std::make_pair(node2, evidence_list));
    }
    if (B.status != HC_BR_OK) return;
    for (auto node_pair : missing_inclusion_edges) {  // :328-335
        evidence_per_neighbor.at(node_pair.first).clear();
        if (neighbors.size() == 2) final_branch.clear();
        else final_branch.remove(node_pair.first);
    }
    auto branch_it = final_branch.begin();
    if (branch_it != final_branch.end()) branch_it++;  // (:349 on an empty list stays at end() in libstdc++)
    for (uint32_t neighbor : neighbors) {
        if (branch_it != final_branch.end() && neighbor == *branch_it) {
            B.stored.push_back(std::make_pair(neighbor, evidence_per_neighbor.at(neighbor)));
            branch_it++;
        }
    }
    if (!final_branch.empty()) final_branch.pop_front();
    B.final_branch = final_branch;
}

void failed(Branch& B) {  // a failed branch contributes nothing
    B.is_false = false;
    B.dist = 0;
    B.final_branch.clear();
    B.diff_list.clear();
    B.missing_edges.clear();
    B.stored.clear();
}

}  // namespace

extern "C" int hc_host_br_evidence(const hc_br_host_input* in, const hc_br_settings* st, hc_br_counts* counts, hc_br_tables* tables, uint32_t n_threads) {
    if (!in || !st || !counts) return fail(HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    const uint64_t V = in->n_vertices;
    if (!in->out_off || !in->in_off || !in->seq_off || !in->read_first_seq || !in->orig_off || (V && (!in->vertex_read || !in->vertex_fwd)))
        return fail(HC_ERR_ARG, "null array");
    if (V >= (1ull << 31)) return fail(HC_ERR_ARG, "2^31 vertices or more");
    const uint64_t E = in->out_off[V];
    if (in->in_off[V] != E || (E && (!in->edges || !in->in_nodes))) return fail(HC_ERR_ARG, "adj_in and adj_out differ in size, or a null array");
    if (const char* what = hc::br::check_original_reads(in->original_bases, in->original_seq_off, in->n_original_reads)) return fail(HC_ERR_ARG, what);
    if (const char* what = hc::br::check_settings(st, in->n_original_reads)) return fail(HC_ERR_ARG, what);
    for (uint64_t v = 0; v < V; v++)
        if (in->vertex_read[v] >= in->n_reads) return fail(HC_ERR_ARG, "a vertex_read is no read of the store");
    View g{in, st, {}, {}};
    g.order.resize(E);
    g.sorted_in.assign(in->in_nodes, in->in_nodes + E);
    {
        std::vector<uint32_t> targets, perm;
        for (uint64_t v = 0; v < V; v++) {
            const uint64_t a = in->out_off[v], n = in->out_off[v + 1] - a;
            targets.resize(n), perm.resize(n);
            for (uint64_t k = 0; k < n; k++) targets[k] = (uint32_t)in->edges[a + k].v2;
            hc::target_sort_perm(targets.data(), n, perm.data());
            for (uint64_t k = 0; k < n; k++) g.order[a + k] = (uint32_t)(a + perm[k]);
            std::sort(g.sorted_in.begin() + in->in_off[v], g.sorted_in.begin() + in->in_off[v + 1]);
        }
    }
    // :60-80: branch_in, then branch_out, each in ascending vertex (std::set order)
    std::vector<Branch> branches;
    for (int side = 0; side < 2; side++)
        for (uint64_t v = 0; v < V; v++) {
            const uint64_t n = side ? in->out_off[v + 1] - in->out_off[v] : in->in_off[v + 1] - in->in_off[v];
            if (n > 1) {
                Branch B;
                B.node = (uint32_t)v, B.outbranch = side != 0, B.n_neighbours = (uint32_t)n;
                branches.push_back(B);
            }
        }
    auto run = [&](size_t first, size_t last) {
        std::vector<uint32_t> neighbors;
        for (size_t b = first; b < last; b++) {
            Branch& B = branches[b];
            neighbors.clear();
            if (B.outbranch)
                for (uint64_t k = in->out_off[B.node]; k < in->out_off[B.node + 1]; k++) neighbors.push_back((uint32_t)in->edges[g.order[k]].v2);
            else
                neighbors.assign(g.sorted_in.begin() + in->in_off[B.node], g.sorted_in.begin() + in->in_off[B.node + 1]);
            find_branching_evidence(g, B, neighbors);
            if (B.status != HC_BR_OK) failed(B);
        }
    };
    const size_t nb = branches.size(), nt = std::max<size_t>(1, std::min<size_t>(n_threads, nb));
    if (nt <= 1) {
        run(0, nb);
    } else {
        std::vector<std::thread> pool;
        for (size_t t = 0; t < nt; t++) pool.emplace_back(run, nb * t / nt, nb * (t + 1) / nt);
        for (std::thread& th : pool) th.join();
    }
    // evidence_per_edge, :347-391, in the order of the calls
    std::map<std::pair<uint32_t, uint32_t>, std::list<uint32_t>> evidence_per_edge;
    for (const Branch& B : branches) {
        if (B.arg_error) return fail(HC_ERR_ARG, "a neighbour's record is missing from adj_out or names a read that is no read of the store");
        for (const auto& s : B.stored) {
            const std::pair<uint32_t, uint32_t> index = B.outbranch ? std::make_pair(B.node, s.first) : std::make_pair(s.first, B.node);
            auto ev_it = evidence_per_edge.find(index);
            if (ev_it != evidence_per_edge.end()) {
                std::list<uint32_t> intersection;
                for (uint32_t id : ev_it->second)
                    if (std::find(s.second.begin(), s.second.end(), id) != s.second.end()) intersection.push_back(id);
                ev_it->second = intersection;
            } else {
                evidence_per_edge.insert(std::make_pair(index, s.second));
            }
        }
    }
    for (const Branch& B : branches) {
        counts->n_branch_nb += B.final_branch.size();
        counts->n_diff += B.diff_list.size();
        counts->n_missing += B.missing_edges.size();
        counts->n_items += B.status == HC_BR_OK || B.status == HC_BR_BAD_ORIGINAL ? B.n_items : 0;
        counts->n_failed += B.status != HC_BR_OK;
    }
    counts->n_branches = nb;
    counts->n_ev_edges = evidence_per_edge.size();
    for (const auto& e : evidence_per_edge) counts->n_ev_ids += e.second.size();
    if (!tables) return counts->n_failed ? HC_BR_SOME_FAILED : HC_OK;
    const hc_br_tables& T = *tables;
    if ((T.branches && T.cap_branches < nb) || (T.branch_nb && T.cap_branch_nb < counts->n_branch_nb) || (T.diff_pos && T.cap_diff < counts->n_diff) ||
        ((T.ev_edge || T.ev_off) && T.cap_ev_edges < counts->n_ev_edges) || (T.ev_ids && T.cap_ev_ids < counts->n_ev_ids) ||
        (T.missing_edges && T.cap_missing < counts->n_missing))
        return fail(HC_ERR_ARG, "a table is too small (the counts are filled)");
    uint64_t n_nb = 0, n_diff = 0, n_missing = 0;
    for (size_t b = 0; b < nb; b++) {
        const Branch& B = branches[b];
        if (T.branches) {
            hc_br_branch r;
            memset(&r, 0, sizeof r);
            r.node = B.node, r.side = B.outbranch ? HC_BR_OUT : HC_BR_IN, r.status = B.status, r.is_false = B.is_false, r.dist = B.dist;
            r.nb_first = n_nb, r.nb_count = (uint32_t)B.final_branch.size();
            r.diff_first = n_diff, r.diff_count = (uint32_t)B.diff_list.size();
            r.n_neighbours = B.n_neighbours;
            T.branches[b] = r;
        }
        for (uint32_t x : B.final_branch) {
            if (T.branch_nb) T.branch_nb[n_nb] = x;
            n_nb++;
        }
        for (int x : B.diff_list) {
            if (T.diff_pos) T.diff_pos[n_diff] = x;
            n_diff++;
        }
        for (const hc_edge_rec& e : B.missing_edges) {
            if (T.missing_edges) T.missing_edges[n_missing] = e;
            n_missing++;
        }
    }
    uint64_t k = 0, n_ids = 0;
    for (const auto& e : evidence_per_edge) {
        if (T.ev_edge) T.ev_edge[2 * k] = e.first.first, T.ev_edge[2 * k + 1] = e.first.second;
        if (T.ev_off) T.ev_off[k] = n_ids;
        for (uint32_t id : e.second) {
            if (T.ev_ids) T.ev_ids[n_ids] = id;
            n_ids++;
        }
        k++;
    }
    if (T.ev_off) T.ev_off[k] = n_ids;
    return counts->n_failed ? HC_BR_SOME_FAILED : HC_OK;
}
