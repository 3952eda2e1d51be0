// Cliques.cpp — hc_host_graph_cliques (include/hcedge_host.h), the host mirror of hc_graph_cliques, and host_root, the per-root
// routine both use (the device call for its roots above root_cap).  The graph is the one OverlapGraph::writeGraphToFile describes
// (reference src/OverlapGraph.cpp:322-385); the order is the rule of CliqueRule.h, whose expressions decide here as on the device.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/hcedge_host.h"
#include "../hc_cliques.h"
#include "../hc_scratch.h"

namespace hc {
namespace cliques {

bool host_root(const HostAdj& a, uint32_t v, uint64_t budget, std::vector<uint32_t>& sizes, std::vector<uint32_t>& nodes, uint64_t* entries,
               uint32_t* max_clique) {
    const uint32_t* N = a.nbr + a.off[v];
    const uint32_t d = (uint32_t)(a.off[v + 1] - a.off[v]), W = words_of(d);
    if (d == 0) {  // P = {} and X = {}
        sizes.push_back(1);
        nodes.push_back(v);
        *entries += 1;
        *max_clique = std::max(*max_clique, 1u);
        return *entries <= budget;
    }
    uint32_t n_P = 0;
    for (uint32_t b = 0; b < d; b++) n_P += starts_in_P(a.rank[N[b]], a.rank[v]);
    if (!n_P) return true;  // P = {} and X != {}: v's cliques belong to roots of smaller rank
    std::vector<uint64_t> stack(((size_t)n_P + 1) * 3 * W, 0), R(W, 0);  // (a level takes a vertex out of P: |P| + 1 levels)
    std::vector<uint32_t> cur((size_t)n_P + 1);
    for (uint32_t b = 0; b < d; b++) stack[(starts_in_P(a.rank[N[b]], a.rank[v]) ? 0 : W) + (b >> 6)] |= 1ull << (b & 63u);
    std::vector<uint64_t> M((size_t)d * W);
    for (uint32_t b = 0; b < d; b++) matrix_row(a.nbr + a.off[N[b]], (uint32_t)(a.off[N[b] + 1] - a.off[N[b]]), N, d, M.data() + (size_t)b * W);
    const uint32_t lt = (uint32_t)(std::lower_bound(N, N + d, v) - N);
    uint32_t level = 0;
    bool entering = true;
    for (;;) {
        uint64_t* P = stack.data() + (size_t)level * 3 * W;
        uint64_t *X = P + W, *C = X + W;
        bool pop = false;
        if (entering) {
            bool any_P = false, any_X = false;
            for (uint32_t w = 0; w < W; w++) any_P |= P[w] != 0, any_X |= X[w] != 0;
            if (!any_P) {
                if (emits(any_P, any_X)) {
                    bool placed = false;
                    for (uint32_t w = 0; w < W; w++)
                        for (uint64_t word = R[w]; word; word &= word - 1) {
                            const uint32_t b = w * 64 + (uint32_t)__builtin_ctzll(word);
                            if (!placed && b >= lt) nodes.push_back(v), placed = true;
                            nodes.push_back(N[b]);
                        }
                    if (!placed) nodes.push_back(v);
                    sizes.push_back(level + 1);
                    *entries += level + 1;
                    *max_clique = std::max(*max_clique, level + 1);
                    if (*entries > budget) return false;
                }
                pop = true;
            } else {
                uint64_t best = 0;
                for (uint32_t w = 0; w < W; w++)
                    for (uint64_t word = P[w] | X[w]; word; word &= word - 1) {
                        const uint32_t u = w * 64 + (uint32_t)__builtin_ctzll(word);
                        uint32_t score = 0;
                        for (uint32_t w2 = 0; w2 < W; w2++) score += (uint32_t)__builtin_popcountll(M[(size_t)u * W + w2] & P[w2]);
                        best = std::max(best, pivot_key(score, u));
                    }
                const uint64_t* prow = M.data() + (size_t)pivot_of(best) * W;
                for (uint32_t w = 0; w < W; w++) C[w] = candidates(P[w], prow[w]);
            }
            entering = false;
        }
        if (!pop) {
            uint32_t w = 0;
            while (w < W && !C[w]) w++;
            if (w == W) {
                pop = true;
            } else {
                const uint32_t b = w * 64 + (uint32_t)__builtin_ctzll(C[w]);
                C[w] &= C[w] - 1;
                const uint64_t* row = M.data() + (size_t)b * W;
                for (uint32_t w2 = 0; w2 < W; w2++) P[3 * W + w2] = P[w2] & row[w2], P[4 * W + w2] = X[w2] & row[w2];
                cur[level] = b;
                R[b >> 6] |= 1ull << (b & 63u);
                level++;
                entering = true;
                continue;
            }
        }
        if (level == 0) break;
        level--;
        const uint32_t b = cur[level];
        uint64_t* P0 = stack.data() + (size_t)level * 3 * W;
        R[b >> 6] &= ~(1ull << (b & 63u));
        P0[b >> 6] &= ~(1ull << (b & 63u));
        P0[W + (b >> 6)] |= 1ull << (b & 63u);
    }
    return true;
}

}  // namespace cliques
}  // namespace hc

namespace {
int fail(int status, const std::string& what) { return hc::set_last_error(status, "hc_host_graph_cliques: " + what); }
struct Root {
    std::vector<uint32_t> sizes, nodes;
};
}  // namespace

extern "C" int hc_host_graph_cliques(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, const uint8_t* inclusions,
                                     const hc_cliques_settings* st, uint64_t* clique_off, uint32_t* clique_nodes, uint64_t cap_cliques,
                                     uint64_t cap_entries, hc_cliques_counts* counts) {
    namespace cl = hc::cliques;
    constexpr uint64_t kLimit = 1ull << 31;
    if (!st || !counts || !out_off) return fail(HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    const uint64_t V = n_vertices;
    if (V >= kLimit || out_off[0] != 0 || out_off[V] >= kLimit || (out_off[V] && !edges)) return fail(HC_ERR_ARG, "not a graph hc_graph_fetch returns");
    const uint64_t budget = st->max_entries ? st->max_entries : kLimit - 1;
    if (budget >= kLimit) return fail(HC_ERR_ARG, "max_entries is not below 2^31");
    const auto t0 = std::chrono::steady_clock::now();
    // writeGraphToFile's loops: the asserts in file order, the pairs
    std::vector<uint64_t> keys;
    for (uint64_t i = 0; i < V; i++) {
        if (out_off[i + 1] < out_off[i] || out_off[i + 1] > out_off[V]) return fail(HC_ERR_ARG, "out_off descends");
        if (inclusions && inclusions[i]) {
            if (out_off[i + 1] != out_off[i]) {  // :346
                counts->status = HC_CLIQUES_INCLUSION_HAS_EDGES, counts->bad_v = i;
                return HC_OK;
            }
            continue;
        }
        for (uint64_t k = out_off[i]; k < out_off[i + 1]; k++) {
            const uint64_t j = edges[k].v2;
            if (j >= V) return fail(HC_ERR_ARG, "a target is not a vertex");
            if (inclusions && inclusions[j]) continue;  // :352
            if (j == i) {                               // :355
                counts->status = HC_CLIQUES_SELF_LOOP, counts->bad_v = i, counts->bad_pos = k - out_off[i];
                return HC_OK;
            }
            keys.push_back(i << 32 | j);
            keys.push_back(j << 32 | i);
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.size() >= kLimit) return fail(HC_ERR_ARG, "2 * n_pairs is not below 2^31");
    counts->n_pairs = keys.size() / 2;
    std::vector<uint64_t> off(V + 1, 0), rank_keys(V);
    std::vector<uint32_t> nbr(keys.size()), rank(V), order(V);
    for (size_t k = 0; k < keys.size(); k++) off[(keys[k] >> 32) + 1]++, nbr[k] = (uint32_t)keys[k];
    for (uint64_t v = 0; v < V; v++) rank_keys[v] = cl::rank_key((uint32_t)off[v + 1], (uint32_t)v), off[v + 1] += off[v];
    std::sort(rank_keys.begin(), rank_keys.end());
    for (uint64_t r = 0; r < V; r++) order[r] = (uint32_t)rank_keys[r], rank[order[r]] = (uint32_t)r;
    // the roots, by ticket; the budget is tested after every root and inside one
    const cl::HostAdj adj{off.data(), nbr.data(), rank.data()};
    std::vector<Root> roots(V);
    std::atomic<uint64_t> next{0}, total{0};
    std::atomic<uint32_t> biggest{0};
    std::atomic<bool> stop{false};
    auto work = [&]() {
        uint32_t mine = 0;
        for (uint64_t r; !stop.load() && (r = next.fetch_add(1)) < V;) {
            uint64_t entries = 0;
            const bool ok = cl::host_root(adj, order[r], budget, roots[r].sizes, roots[r].nodes, &entries, &mine);
            if (!ok || total.fetch_add(entries) + entries > budget) stop.store(true);
        }
        uint32_t seen = biggest.load();
        while (mine > seen && !biggest.compare_exchange_weak(seen, mine)) {
        }
    };
    const uint32_t nt = st->n_threads ? st->n_threads : 1;
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt && t < V; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    counts->ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stop.load()) {
        counts->status = HC_CLIQUES_OVER_BUDGET;
        return HC_OK;
    }
    uint64_t n_cliques = 0, n_entries = 0;
    for (uint64_t r = 0; r < V; r++) {
        n_cliques += roots[r].sizes.size(), n_entries += roots[r].nodes.size();
        if (off[order[r] + 1] == off[order[r]]) counts->n_singletons++;
    }
    if (n_cliques >= kLimit || n_entries >= kLimit) return fail(HC_ERR_ARG, "n_cliques or n_entries is not below 2^31");
    counts->n_cliques = n_cliques, counts->n_entries = n_entries, counts->max_clique = biggest.load();
    if (!clique_off && !clique_nodes) return HC_OK;  // the count of count-then-fetch
    if ((clique_off && cap_cliques < n_cliques) || (clique_nodes && cap_entries < n_entries)) return fail(HC_ERR_ARG, "the cliques do not fit the buffers");
    uint64_t c = 0, e = 0;
    for (uint64_t r = 0; r < V; r++) {
        if (clique_nodes && !roots[r].nodes.empty()) memcpy(clique_nodes + e, roots[r].nodes.data(), roots[r].nodes.size() * 4);
        for (uint32_t sz : roots[r].sizes) {
            if (clique_off) clique_off[c] = e;
            c++, e += sz;
        }
    }
    if (clique_off) clique_off[c] = e;
    counts->ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return HC_OK;
}
