// Cycles.cpp — OverlapGraph::cycleRemovalHeuristic on the host: the pieces hc_graph_remove_cycles shares with the mirror (Cycles.h) and
// the mirror itself, a restatement of src/GraphAlgos.cpp:150-176, 352-541 and src/OverlapGraph.cpp:104-147, 548-562 over hc_graph_fetch's
// flat arrays.
#include "Cycles.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>

#include "../../../include/hcedge_host.h"
#include "Labelling.h"
#include "Types.h"

namespace hc {
int set_last_error(int status, const std::string& what);  // hc_api.cpp (or the sanitizer build's stub)

namespace cycles {

void walk(const uint32_t* roots, uint64_t n_roots, const uint64_t* off, const uint32_t* col, uint32_t V, std::vector<uint64_t>& pairs) {
    pairs.clear();
    std::vector<uint8_t> state(V, 0);  // 1: marked (on the current path), 2: visited
    struct Frame {
        uint32_t node;
        uint64_t next;
    };
    std::vector<Frame> stack;
    for (uint64_t i = 0; i < n_roots; i++) {
        const uint32_t root = roots[i];
        if (state[root]) continue;  // (nothing is marked between two roots: only `visited` can be set)
        state[root] = 1;
        stack.push_back(Frame{root, off[root]});
        while (!stack.empty()) {
            Frame& f = stack.back();
            if (f.next < off[f.node + 1]) {
                const uint32_t w = col[f.next++];
                if (state[w] == 1) {  // :356-358
                    pairs.push_back((uint64_t)f.node << 32 | w);
                } else if (state[w] == 0) {  // :371-373
                    state[w] = 1;
                    stack.push_back(Frame{w, off[w]});  // (f is dead from here)
                }
            } else {  // :480-483
                state[f.node] = 2;
                stack.pop_back();
            }
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
}

void roots_by_indegree(const uint64_t* in_off, uint32_t V, std::vector<uint32_t>& roots) {
    roots.resize(V);
    for (uint32_t v = 0; v < V; v++) roots[v] = v;
    std::stable_sort(roots.begin(), roots.end(), [&](uint32_t a, uint32_t b) { return in_off[a + 1] - in_off[a] < in_off[b + 1] - in_off[b]; });
}

namespace {
template <typename K, typename Less>
void sorted_targets(const hc_edge_rec* list, size_t n, K key_of(const hc_edge_rec&), Less before, uint32_t* out) {
    std::vector<std::pair<uint32_t, K>> pairs;
    pairs.reserve(n);
    for (size_t k = 0; k < n; k++) pairs.push_back(std::make_pair((uint32_t)list[k].v2, key_of(list[k])));
    std::sort(pairs.begin(), pairs.end(), [&](const std::pair<uint32_t, K>& a, const std::pair<uint32_t, K>& b) {
        if (a.second == b.second) return a.first < b.first;
        return before(a.second, b.second);
    });
    for (size_t k = 0; k < n; k++) out[k] = pairs[k].first;
}
int key_pos1(const hc_edge_rec& e) { return e.pos1; }
int key_len0(const hc_edge_rec& e) { return e.len0; }
double key_score(const hc_edge_rec& e) { return e.score; }
double key_mismatch(const hc_edge_rec& e) { return e.mismatch_rate; }
}  // namespace

void target_column(const hc_edge_rec* edges, const uint64_t* out_off, uint32_t V, uint32_t t, std::vector<uint32_t>& col) {
    col.resize(out_off[V]);
    label::ShuffleCache shuffles(t);
    for (uint32_t v = 0; v < V; v++) {
        const hc_edge_rec* list = edges + out_off[v];
        const size_t n = out_off[v + 1] - out_off[v];
        uint32_t* out = col.data() + out_off[v];
        if (t == 1) sorted_targets<int>(list, n, key_pos1, [](int a, int b) { return a < b; }, out);                  // :379-400
        else if (t == 2) sorted_targets<double>(list, n, key_score, [](double a, double b) { return a > b; }, out);   // :401-422
        else if (t == 3) sorted_targets<int>(list, n, key_len0, [](int a, int b) { return a > b; }, out);             // :423-444
        else if (t == 4) sorted_targets<double>(list, n, key_mismatch, [](double a, double b) { return a < b; }, out);  // :445-466
        else {  // :467-474
            const std::vector<uint32_t>& perm = shuffles.get((uint32_t)n);
            for (size_t k = 0; k < n; k++) out[k] = (uint32_t)list[perm[k]].v2;
        }
    }
}

void perm_table(uint32_t len, uint32_t* table) {
    std::vector<uint32_t> perm;
    for (uint32_t t = kFirstShuffle; t <= kTries; t++) {
        label::shuffle_permutation(t, len, perm);
        if (len) memcpy(table + (size_t)(t - kFirstShuffle) * len, perm.data(), (size_t)len * 4);
    }
}

void walk_tries(const uint32_t* roots, uint64_t n_roots, const uint64_t* off, const uint32_t* const* cols, uint32_t V, uint32_t first, uint32_t last,
                unsigned n_threads, std::vector<uint64_t>* sets) {
    if (last < first) return;
    std::atomic<uint32_t> next{first};
    std::atomic<bool> failed{false};
    auto work = [&]() {
        try {
            for (uint32_t t; (t = next.fetch_add(1)) <= last;) walk(roots, n_roots, off, cols[t - first], V, sets[t - first]);
        } catch (...) {
            failed.store(true);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < n_threads && t < last - first + 1; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (failed.load()) throw FatalError{HC_ERR_NOMEM, "findCycles: a walk ran out of memory"};
}

void sort_out_list(hc_edge_rec* list, uint32_t* seq, size_t n, const uint32_t* len_by_read) {
    if (n < 2) return;
    struct Key {
        unsigned int nonoverlap;  // src/Edge.h:58-63, unsigned arithmetic
        uint64_t v2;
        uint32_t at;
    };
    std::vector<Key> keys;
    keys.reserve(n);
    for (size_t k = 0; k < n; k++)
        keys.push_back(Key{(unsigned int)len_by_read[list[k].read1] + (unsigned int)len_by_read[list[k].read2] - 2u * (unsigned int)list[k].len0,
                           list[k].v2, (uint32_t)k});
    // the comparator of :733-742 on the same sequence: std::sort's result depends on the comparisons only
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        if (a.nonoverlap == b.nonoverlap) return a.v2 < b.v2;
        return a.nonoverlap < b.nonoverlap;
    });
    std::vector<hc_edge_rec> sorted;
    std::vector<uint32_t> sorted_seq;
    sorted.reserve(n);
    for (const Key& k : keys) {
        sorted.push_back(list[k.at]);
        if (seq) sorted_seq.push_back(seq[k.at]);
    }
    std::copy(sorted.begin(), sorted.end(), list);
    if (seq) std::copy(sorted_seq.begin(), sorted_seq.end(), seq);
}

}  // namespace cycles
}  // namespace hc

// ---- the mirror ------------------------------------------------------------------------------------------------------------

namespace {
namespace cy = hc::cycles;

int check_arrays(const char* me, const hc_edge_rec* edges, const uint64_t* out_off, const uint64_t* in_off, uint64_t V) {
    if (!out_off || !in_off) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": null offsets");
    if (V >= (1ull << 31) || out_off[V] >= (1ull << 31)) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": more than 2^31-1 edges or vertices");
    if (out_off[0] != 0 || in_off[0] != 0 || in_off[V] != out_off[V] || (out_off[V] && !edges))
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": offsets do not span the edges");
    for (uint64_t v = 0; v < V; v++)
        if (out_off[v + 1] < out_off[v] || in_off[v + 1] < in_off[v]) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": offsets decrease");
    for (uint64_t k = 0; k < out_off[V]; k++)
        if (edges[k].v1 >= V || edges[k].v2 >= V) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": a record leaves the graph");
    return HC_OK;
}
}  // namespace

extern "C" {

int hc_host_graph_find_cycles(const hc_edge_rec* edges, const uint64_t* out_off, const uint64_t* in_off, uint64_t n_vertices, uint32_t t,
                              uint32_t* pairs, uint64_t cap_pairs, uint64_t* n_pairs) {
    const char* me = "hc_host_graph_find_cycles";
    if (!n_pairs || t < 1 || t > cy::kTries) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": null count, or a try outside 1 .. 20");
    *n_pairs = 0;
    if (const int rc = check_arrays(me, edges, out_off, in_off, n_vertices)) return rc;
    try {
        const uint32_t V = (uint32_t)n_vertices;
        std::vector<uint32_t> roots, col;
        std::vector<uint64_t> set;
        cy::roots_by_indegree(in_off, V, roots);
        cy::target_column(edges, out_off, V, t, col);
        cy::walk(roots.data(), V, out_off, col.data(), V, set);
        *n_pairs = set.size();
        for (size_t k = 0; pairs && k < set.size() && k < cap_pairs; k++) pairs[2 * k] = (uint32_t)(set[k] >> 32), pairs[2 * k + 1] = (uint32_t)set[k];
    } catch (const std::bad_alloc&) {
        return hc::set_last_error(HC_ERR_NOMEM, std::string(me) + ": out of memory");
    }
    return HC_OK;
}

int hc_host_cycles_perm_table(uint32_t len, uint32_t* table) {
    if (len && !table) return hc::set_last_error(HC_ERR_ARG, "hc_host_cycles_perm_table: null");
    cy::perm_table(len, table);
    return HC_OK;
}

int hc_host_graph_remove_cycles(const hc_edge_rec* edges, const uint64_t* out_off, const uint32_t* in_nodes, const uint64_t* in_off,
                                uint64_t n_vertices, const hc_cycles_settings* st, uint32_t n_threads, hc_edge_rec* edges_out,
                                uint64_t* out_off_out, uint32_t* in_nodes_out, uint64_t* in_off_out, hc_edge_rec* removed, uint32_t* pairs,
                                uint64_t cap_pairs, hc_cycles_counts* counts) {
    const char* me = "hc_host_graph_remove_cycles";
    if (!st || !counts) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": null argument");
    memset(counts, 0, sizeof *counts);
    if (const int rc = check_arrays(me, edges, out_off, in_off, n_vertices)) return rc;
    const uint32_t V = (uint32_t)n_vertices;
    const uint64_t E = out_off[V];
    if (E && !in_nodes) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": null in-lists");
    counts->edges_before = counts->edges_after = E;
    auto copy_graph = [&]() {
        if (edges_out && E) memcpy(edges_out, edges, E * sizeof(hc_edge_rec));
        if (in_nodes_out && E) memcpy(in_nodes_out, in_nodes, E * 4);
        if (out_off_out) memcpy(out_off_out, out_off, (V + 1ull) * 8);
        if (in_off_out) memcpy(in_off_out, in_off, (V + 1ull) * 8);
    };
    try {
        std::vector<uint32_t> roots;
        std::vector<uint64_t> sets[cy::kTries];
        cy::roots_by_indegree(in_off, V, roots);
        {
            std::vector<uint32_t> col;
            cy::target_column(edges, out_off, V, 1, col);
            cy::walk(roots.data(), V, out_off, col.data(), V, sets[0]);
        }
        counts->tries = counts->best_try = 1;
        counts->try_size[0] = sets[0].size();
        if (sets[0].empty()) {  // :517: one try
            copy_graph();
            return HC_OK;
        }
        for (uint32_t v = 0; v < V; v++)
            for (uint64_t k = out_off[v]; k < out_off[v + 1]; k++)
                if (std::isnan(edges[k].score) || std::isnan(edges[k].mismatch_rate)) {
                    counts->status = HC_CYCLES_NAN_KEY, counts->bad_v = v, counts->bad_pos = (uint32_t)(k - out_off[v]);
                    copy_graph();
                    return HC_OK;
                }
        {  // what the device call's compact CSR would hold: the weak components that own a pair of try 1
            std::vector<uint32_t> parent(V);
            for (uint32_t v = 0; v < V; v++) parent[v] = v;
            auto find = [&](uint32_t x) {
                while (parent[x] != x) x = parent[x] = parent[parent[x]];
                return x;
            };
            for (uint64_t k = 0; k < E; k++) {
                const uint32_t a = find((uint32_t)edges[k].v1), b = find((uint32_t)edges[k].v2);
                if (a != b) parent[a > b ? a : b] = a > b ? b : a;
            }
            std::vector<uint8_t> flagged(V, 0);
            for (uint64_t p : sets[0]) flagged[find((uint32_t)(p >> 32))] = 1;
            for (uint32_t v = 0; v < V; v++) {
                if (flagged[v] && parent[v] == v) counts->n_flagged_components++;
                if (flagged[find(v)]) counts->n_host_vertices++, counts->n_host_edges += out_off[v + 1] - out_off[v];
            }
        }
        {  // the other 19 tries, every one over the whole graph
            std::vector<std::vector<uint32_t>> cols(cy::kTries - 1);
            const uint32_t* col_ptr[cy::kTries - 1];
            for (uint32_t t = 2; t <= cy::kTries; t++) {
                cy::target_column(edges, out_off, V, t, cols[t - 2]);
                col_ptr[t - 2] = cols[t - 2].data();
            }
            cy::walk_tries(roots.data(), V, out_off, col_ptr, V, 2, cy::kTries, n_threads ? n_threads : 1, sets + 1);
        }
        counts->tries = cy::kTries;
        uint32_t best = 0;
        for (uint32_t t = 0; t < cy::kTries; t++) {
            counts->try_size[t] = sets[t].size();
            if (sets[t].size() < sets[best].size()) best = t;  // :522: strictly smaller
        }
        counts->best_try = best + 1;
        const std::vector<uint64_t>& opt = sets[best];
        counts->backedge_count = opt.size();
        if (opt.size() > cap_pairs && (pairs || removed)) return hc::set_last_error(HC_ERR_ARG, std::string(me) + ": more pairs than cap_pairs");
        for (size_t k = 0; pairs && k < opt.size(); k++) pairs[2 * k] = (uint32_t)(opt[k] >> 32), pairs[2 * k + 1] = (uint32_t)opt[k];
        if (!st->remove_edges) {
            copy_graph();
            return HC_OK;
        }
        // reportCycle / removeEdge per pair in the set's order: the first record u -> v, the first u of adj_in[v]
        std::vector<uint8_t> gone_out(E, 0), gone_in(E, 0);
        for (size_t k = 0; k < opt.size(); k++) {
            const uint32_t u = (uint32_t)(opt[k] >> 32), v = (uint32_t)opt[k];
            uint64_t q = out_off[u];
            while (q < out_off[u + 1] && (gone_out[q] || edges[q].v2 != v)) q++;
            if (q == out_off[u + 1]) throw hc::FatalError{HC_ERR_STATE, "removeEdge: Edge to be removed not found"};
            gone_out[q] = 1;
            if (removed) removed[k] = edges[q];
            uint64_t p = in_off[v];
            while (p < in_off[v + 1] && (gone_in[p] || in_nodes[p] != u)) p++;
            if (p < in_off[v + 1]) gone_in[p] = 1;  // (:134-145 goes on without it)
        }
        uint64_t n_out = 0, n_in = 0;
        for (uint32_t v = 0; v < V; v++) {
            if (out_off_out) out_off_out[v] = n_out;
            if (in_off_out) in_off_out[v] = n_in;
            for (uint64_t k = out_off[v]; k < out_off[v + 1]; k++)
                if (!gone_out[k]) {
                    if (edges_out) edges_out[n_out] = edges[k];
                    n_out++;
                }
            for (uint64_t k = in_off[v]; k < in_off[v + 1]; k++)
                if (!gone_in[k]) {
                    if (in_nodes_out) in_nodes_out[n_in] = in_nodes[k];
                    n_in++;
                }
        }
        if (out_off_out) out_off_out[V] = n_out;
        if (in_off_out) in_off_out[V] = n_in;
        counts->edges_after = n_out;
    } catch (const hc::FatalError& e) {
        return hc::set_last_error(e.status, std::string(me) + ": " + e.what);
    } catch (const std::bad_alloc&) {
        return hc::set_last_error(HC_ERR_NOMEM, std::string(me) + ": out of memory");
    }
    return HC_OK;
}

}  // extern "C"
