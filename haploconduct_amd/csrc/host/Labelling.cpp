// Labelling.cpp — OverlapGraph::vertexLabellingHeuristic on the host: the mirror (a restatement of src/GraphAlgos.cpp:150-349 and
// src/OverlapGraph.cpp:578-605 over hc::OverlapGraph, statement by statement) and the pieces hc_graph_label_vertices shares with it
// (Labelling.h): the generator behind std::random_shuffle and the BFS tries over the components the device cannot settle.
#include "Labelling.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <thread>
#include <unordered_set>

#include "OverlapGraph.h"
#include "api_helpers.h"

namespace hc {
namespace label {

void GlibcRand::srand(unsigned int seed) {  // glibc srandom_r, TYPE_3
    int32_t word = seed ? (int32_t)seed : 1;
    r_[0] = (uint32_t)word;
    for (int i = 1; i < 31; i++) {  // 16807 * word % 2147483647 without overflow
        const long hi = word / 127773, lo = word % 127773;
        long w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        word = (int32_t)w;
        r_[i] = (uint32_t)word;
    }
    front_ = 3, back_ = 0;
    for (int i = 0; i < 310; i++) rand();
}

void shuffle_permutation(unsigned int seed, uint32_t n, std::vector<uint32_t>& perm) {
    perm.resize(n);
    for (uint32_t i = 0; i < n; i++) perm[i] = i;
    GlibcRand gen(seed);
    for (uint32_t i = 1; i < n; i++) {
        const uint32_t j = (uint32_t)gen.rand() % (i + 1);
        if (i != j) std::swap(perm[i], perm[j]);
    }
}

namespace {
// getEdgeInfo(node, neighbour)'s first hit (src/OverlapGraph.cpp:263-282): node's own list first, then the neighbour's
bool edge_same(const Subgraph& S, uint32_t node, uint32_t nb) {
    for (uint64_t k = S.out_off[node]; k < S.out_off[node + 1]; k++)
        if (S.out_nb[k] == nb) return S.out_same[k] != 0;
    for (uint64_t k = S.out_off[nb]; k < S.out_off[nb + 1]; k++)
        if (S.out_nb[k] == node) return S.out_same[k] != 0;
    throw FatalError{HC_ERR_STATE, "label_tries: a neighbour without an edge"};
}
}  // namespace

void label_tries(const Subgraph& S, uint32_t n_tries, unsigned n_threads, uint64_t* bits) {
    const uint32_t n = S.n;
    memset(bits, 0, (size_t)n * 16);
    if (n == 0 || n_tries == 0) return;
    std::vector<uint32_t> order(n);  // sortVerticesByIndegree, :150-176
    for (uint32_t v = 0; v < n; v++) order[v] = v;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t da = S.in_off[a + 1] - S.in_off[a], db = S.in_off[b + 1] - S.in_off[b];
        return da == db ? a < b : da < db;
    });
    std::mutex merge;
    std::atomic<uint32_t> next{1};
    std::atomic<bool> failed{false};
    auto work = [&]() {
        try {
            std::vector<uint8_t> lab(n), visited(n);
            std::vector<uint32_t> bfs(n), adj_vec;
            for (uint32_t t; (t = next.fetch_add(1)) <= n_tries;) {
                ShuffleCache shuffles(t);
                std::fill(lab.begin(), lab.end(), 1);
                std::fill(visited.begin(), visited.end(), 0);
                for (uint32_t i = 0; i < n; i++) {
                    if (visited[order[i]]) continue;
                    size_t head = 0, tail = 0;
                    bfs[tail++] = order[i];
                    visited[order[i]] = 1;
                    while (head < tail) {
                        const uint32_t node = bfs[head++];
                        adj_vec.assign(S.in_nb + S.in_off[node], S.in_nb + S.in_off[node + 1]);
                        adj_vec.insert(adj_vec.end(), S.out_nb + S.out_off[node], S.out_nb + S.out_off[node + 1]);
                        const std::vector<uint32_t>& perm = shuffles.get((uint32_t)adj_vec.size());
                        for (uint32_t k : perm) {
                            const uint32_t nb = adj_vec[k];
                            if (visited[nb]) continue;
                            bfs[tail++] = nb;
                            visited[nb] = 1;
                            lab[nb] = edge_same(S, node, nb) ? lab[node] : !lab[node];
                        }
                    }
                }
                std::lock_guard<std::mutex> hold(merge);
                const uint64_t bit = 1ull << ((t - 1) & 63);
                for (uint32_t v = 0; v < n; v++)
                    if (lab[v]) bits[2 * (size_t)v + ((t - 1) >> 6)] |= bit;
            }
        } catch (...) {
            failed.store(true);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < n_threads && t < n_tries; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (failed.load()) throw FatalError{HC_ERR_STATE, "label_tries: the subgraph's lists do not match"};
}

}  // namespace label

// ---- the mirror ------------------------------------------------------------------------------------------------------------

struct OverlapGraph::LabelTry {  // edges_to_be_moved / edges_to_be_deleted of one labelVertices call, and where their originals stand
    std::vector<Edge> moved, deleted;
    std::vector<uint64_t> moved_at, deleted_at;  // vertex << 32 | position
    void clear() { moved.clear(), deleted.clear(), moved_at.clear(), deleted_at.clear(); }
};

std::vector<node_id_t> OverlapGraph::sortVerticesByIndegree() const {  // src/GraphAlgos.cpp:150-176
    std::vector<std::pair<node_id_t, unsigned int>> pairs;
    node_id_t v = 0;
    for (const auto& it : adj_in) {
        pairs.push_back(std::make_pair(v, (unsigned int)it.size()));
        v++;
    }
    std::sort(pairs.begin(), pairs.end(), [](const std::pair<node_id_t, unsigned int>& a, const std::pair<node_id_t, unsigned int>& b) {
        if (a.second == b.second) return a.first < b.first;
        return a.second < b.second;
    });
    std::vector<node_id_t> sorted_vertices;
    for (const auto& pair_it : pairs) sorted_vertices.push_back(pair_it.first);
    return sorted_vertices;
}

static Edge* edge_info_either(OverlapGraph& G, node_id_t v, node_id_t w) {  // getEdgeInfo with reverse_allowed, src/OverlapGraph.cpp:263-282
    for (Edge& e : G.adj_out.at(v))
        if (e.get_vertex(2) == w) return &e;
    for (Edge& e : G.adj_out.at(w))
        if (e.get_vertex(2) == v) return &e;
    throw FatalError{HC_ERR_STATE, "getEdgeInfo: Edge not found"};
}

void OverlapGraph::labelVertices(LabelTry& out, std::vector<uint8_t>& orientations, int rand_seed) {  // :250-349
    const size_t V = adj_out.size();
    orientations.resize(V, 1);  // (a vector that has its size keeps its values, as the reference's bitset does)
    std::vector<uint8_t> visited(V, 0);
    std::vector<node_id_t> bfs(V);
    const std::vector<node_id_t> sorted_vertices = sortVerticesByIndegree();
    label::ShuffleCache shuffles((unsigned)rand_seed);  // std::srand(rand_seed); std::random_shuffle(...), :273-274
    std::vector<node_id_t> adj_vec;
    for (size_t i = 0; i < V; i++) {
        const node_id_t start_node = sorted_vertices.at(i);
        size_t head = 0, tail = 0;
        if (!visited[start_node]) {
            bfs[tail++] = start_node;
            visited[start_node] = 1;
        }
        while (head < tail) {
            const node_id_t node = bfs[head++];
            adj_vec.assign(adj_in.at(node).begin(), adj_in.at(node).end());
            for (const Edge& edge_it : adj_out.at(node)) adj_vec.push_back(edge_it.get_vertex(2));
            const std::vector<uint32_t>& perm = shuffles.get((uint32_t)adj_vec.size());
            for (uint32_t k : perm) {
                const node_id_t neighbor_it = adj_vec[k];
                if (!visited[neighbor_it]) {
                    bfs[tail++] = neighbor_it;
                    visited[neighbor_it] = 1;
                    const Edge* edge = edge_info_either(*this, node, neighbor_it);
                    if (edge->get_ori(1) == edge->get_ori(2)) orientations[neighbor_it] = orientations[node];
                    else orientations[neighbor_it] = !orientations[node];
                }
            }
        }
    }
    // check all edges, :294-348
    for (node_id_t i = 0; i < V; i++) {
        auto& list = adj_out[i];
        for (size_t j = 0; j < list.size(); j++) {
            Edge* it2 = &list[j];
            const node_id_t u = it2->get_vertex(1), v = it2->get_vertex(2);
            const bool ori1 = it2->get_ori(1), ori2 = it2->get_ori(2);
            const bool type_v1 = orientations[u], type_v2 = orientations[v];
            if (ori1 == type_v1 && ori2 == type_v2) continue;  // edge ok
            if ((ori1 == ori2 && type_v1 != type_v2) || (ori1 != ori2 && type_v1 == type_v2)) {  // contradiction
                out.deleted.push_back(*it2);
                out.deleted_at.push_back((uint64_t)i << 32 | j);
            } else {  // the edge agrees with the labelling but the read orientations need to be flipped
                Edge edge = *it2;
                const bool move = edge.switch_edge_orientation();
                if (move) {
                    out.moved.push_back(edge);
                    out.moved_at.push_back((uint64_t)i << 32 | j);
                } else {
                    it2->switch_edge_orientation();
                }
            }
        }
    }
}

void OverlapGraph::vertexLabellingHeuristic(const hc_label_settings& st, hc_label_counts& c) {  // :178-248
    memset(&c, 0, sizeof c);
    const size_t V = adj_out.size();
    c.edges_before = c.edges_after = edge_count;
    std::vector<uint8_t> opt_orientations(V, 1);
    if (st.flags & HC_FLAG_ADD_DUPLICATES) {
        for (node_id_t i = st.n_reads; i < V; i++) opt_orientations[i] = 0;
    } else if (st.flags & HC_FLAG_RESOLVE_ORIENTATIONS) {
        // the refusal: removeEdgeWithOri's "first match" must be the record that was classified
        std::vector<std::vector<uint8_t>> ori_before(V);
        for (node_id_t v = 0; v < V; v++) {
            const auto& list = adj_out[v];
            std::unordered_set<uint64_t> seen;
            ori_before[v].resize(list.size());
            for (size_t j = 0; j < list.size(); j++) {
                ori_before[v][j] = list[j].get_ori(1);
                if (!seen.insert((uint64_t)list[j].get_vertex(2) << 1 | (list[j].get_ori(1) == list[j].get_ori(2))).second) {
                    c.status = HC_LABEL_REPEATED_RECORD, c.bad_v = (uint32_t)v, c.bad_pos = (uint32_t)j;
                    return;
                }
            }
        }
        {  // components over the doubled vertex set: 2 v + p is "v with parity p"
            std::vector<uint32_t> parent(2 * V);
            for (size_t x = 0; x < 2 * V; x++) parent[x] = (uint32_t)x;
            auto find = [&](uint32_t x) {
                while (parent[x] != x) x = parent[x] = parent[parent[x]];
                return x;
            };
            auto unite = [&](uint32_t a, uint32_t b) {
                a = find(a), b = find(b);
                if (a != b) parent[a > b ? a : b] = a > b ? b : a;
            };
            for (const auto& list : adj_out)
                for (const Edge& e : list) {
                    const uint32_t u = (uint32_t)e.get_vertex(1), v = (uint32_t)e.get_vertex(2), x = e.get_ori(1) == e.get_ori(2) ? 0 : 1;
                    unite(2 * u, 2 * v + x), unite(2 * u + 1, 2 * v + (1 - x));
                }
            std::unordered_set<uint32_t> comps, odd;
            for (size_t v = 0; v < V; v++) {
                const uint32_t a = find(2 * (uint32_t)v), b = find(2 * (uint32_t)v + 1);
                comps.insert(a < b ? a : b);
                if (a == b) odd.insert(a);
            }
            c.n_components = comps.size(), c.n_inconsistent = odd.size();
        }
        LabelTry min_edges, edges;
        labelVertices(min_edges, opt_orientations, 1);
        size_t delete_count = min_edges.deleted.size();
        std::vector<uint8_t> orientations;
        int count = 1;
        c.best_try = 1;
        while (count < 100 && delete_count > 0) {  // k = 100 tries
            count++;
            labelVertices(edges, orientations, count);
            if (edges.deleted.size() < delete_count) {
                min_edges = edges;
                delete_count = min_edges.deleted.size();
                opt_orientations = orientations;
                c.best_try = count;
            }
            edges.clear();
        }
        c.tries = count;
        c.n_moved = min_edges.moved.size();
        {  // records that stay where they are and ended up switched
            std::unordered_set<uint64_t> leaving(min_edges.moved_at.begin(), min_edges.moved_at.end());
            leaving.insert(min_edges.deleted_at.begin(), min_edges.deleted_at.end());
            for (node_id_t v = 0; v < V; v++)
                for (size_t j = 0; j < adj_out[v].size(); j++)
                    if (adj_out[v][j].get_ori(1) != (bool)ori_before[v][j] && !leaving.count((uint64_t)v << 32 | j)) c.n_switched++;
        }
        for (const Edge& edge_it : min_edges.moved) {  // move edges, :220-226
            const node_id_t u = edge_it.get_vertex(1), v = edge_it.get_vertex(2);
            const bool opposite_ori = edge_it.get_ori(1) == edge_it.get_ori(2);
            removeEdgeWithOri(v, u, opposite_ori);
            addEdge(edge_it);
        }
        if (delete_count > 0) {  // remove edges that were conflicting, :227-239
            c.conflict_count = delete_count;
            for (const Edge& edge_it : min_edges.deleted) {
                const node_id_t u = edge_it.get_vertex(1), v = edge_it.get_vertex(2);
                const bool opposite_ori = edge_it.get_ori(1) == edge_it.get_ori(2);
                removeEdgeWithOri(u, v, opposite_ori);
            }
        }
    }
    vertex_orientations = opt_orientations;
    c.edges_after = edge_count;
    // checkDuplicateEdges, src/OverlapGraph.cpp:578-605
    for (node_id_t i = 0; i < V; i++) {
        node_id_t j_prev = 0;
        for (size_t k = 0; k < adj_out[i].size(); k++) {
            const node_id_t j = adj_out[i][k].get_vertex(2);
            if (k != 0 && j == j_prev) {
                c.status = HC_LABEL_DUPLICATE_EDGE, c.bad_v = (uint32_t)i, c.bad_pos = (uint32_t)k;
                return;
            }
            j_prev = j;
        }
    }
}

}  // namespace hc

// ---- C entry points (include/hcedge_host.h) ----------------------------------------------------------------------------------

extern "C" {

int hc_host_graph_label_vertices(hc_host_graph* g, const hc_label_settings* settings, hc_label_counts* counts) {
    if (!g || !settings || !counts) return set_last_error(HC_ERR_ARG, "hc_host_graph_label_vertices: null");
    memset(counts, 0, sizeof *counts);
    return guarded("vertexLabellingHeuristic", [&] { g->graph->vertexLabellingHeuristic(*settings, *counts); });
}

int hc_host_graph_get_orientations(hc_host_graph* g, uint8_t* vertex_fwd, uint64_t n_vertices) {
    if (!g || (n_vertices && !vertex_fwd)) return set_last_error(HC_ERR_ARG, "hc_host_graph_get_orientations: null");
    if (n_vertices != g->graph->adj_out.size()) return set_last_error(HC_ERR_ARG, "hc_host_graph_get_orientations: one byte per vertex");
    const auto& o = g->graph->vertex_orientations;
    for (uint64_t v = 0; v < n_vertices; v++) vertex_fwd[v] = v < o.size() ? o[v] : 1;
    return HC_OK;
}

int hc_host_label_rand(uint32_t seed, int32_t* out, uint64_t n) {
    if (n && !out) return set_last_error(HC_ERR_ARG, "hc_host_label_rand: null");
    hc::label::GlibcRand gen(seed);
    for (uint64_t i = 0; i < n; i++) out[i] = gen.rand();
    return HC_OK;
}

int hc_host_label_shuffle(uint32_t seed, uint32_t* perm, uint64_t n) {
    if ((n && !perm) || n >= (1ull << 32)) return set_last_error(HC_ERR_ARG, "hc_host_label_shuffle: null, or 2^32 elements and more");
    return guarded("shuffle_permutation", [&] {
        std::vector<uint32_t> p;
        hc::label::shuffle_permutation(seed, (uint32_t)n, p);
        if (n) memcpy(perm, p.data(), n * 4);
    });
}

}  // extern "C"
