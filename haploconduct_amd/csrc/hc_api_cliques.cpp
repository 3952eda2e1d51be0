// hc_api_cliques.cpp — hc_graph_cliques and hc_graph_cliques_fetch (include/hcedge.h): the maximal cliques of the graph the context
// holds, kept on the device as a CSR.  The pairs, the simple adjacency and the rank (hc_cliques_kernels.hip over hc_prims.hip's sort,
// unique and sum); the counters back to the host, which refuses a failed assert and sizes the waves' scratch for min(root_cap, the
// largest degree); the count pass; the roots above root_cap on host threads (host/Cliques.cpp: host_root) from the fetched adjacency,
// their counts spliced in; two exclusive sums; the write pass, and the host roots' cliques copied to their places.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hcedge.h"
#include "hc_cliques.h"
#include "hc_ctx.h"
#include "hc_graph_text.h"
#include "hc_prims.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {
constexpr uint64_t kLimit = 1ull << 31;

struct HostRoot {
    uint32_t r;
    std::vector<uint32_t> sizes, nodes;
    uint64_t entries = 0;
    uint32_t biggest = 0;
};
}  // namespace

extern "C" {

int hc_graph_cliques(hc_ctx* c, const hc_cliques_settings* st, hc_cliques_counts* counts) {
    namespace cl = hc::cliques;
    const std::string me = "hc_graph_cliques: ";
    if (!c || !st || !counts) return fail(HC_ERR_ARG, me + "null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::Graph& g = c->graph;
    hc_ctx::Cliques& Q = c->cliques;
    Q.drop();
    if (!g.valid) return fail(HC_ERR_STATE, me + "no graph on the device");
    const uint64_t budget = st->max_entries ? st->max_entries : kLimit - 1;
    if (budget >= kLimit) return fail(HC_ERR_ARG, me + "max_entries is not below 2^31");
    const uint32_t cap = !st->root_cap ? HC_CLIQUES_DEFAULT_ROOT_CAP : st->root_cap < HC_CLIQUES_MAX_ROOT_CAP ? st->root_cap : HC_CLIQUES_MAX_ROOT_CAP;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t V = g.n_vertices, E = g.n_edges, n_keys = 2 * E;
    const uint32_t shift = cl::key_shift(V);
    size_t temp_bytes = hc::prims::sort_temp_bytes(n_keys > V ? n_keys : V, sizeof(uint64_t), 0);
    const size_t select_bytes = hc::prims::select_temp_bytes(n_keys), scan_bytes = hc::prims::scan_temp_bytes(V + 1, sizeof(uint64_t));
    temp_bytes = temp_bytes > select_bytes ? temp_bytes : select_bytes;
    temp_bytes = temp_bytes > scan_bytes ? temp_bytes : scan_bytes;
    int rc;
    if ((rc = Q.keys_a.ensure((n_keys + 1) * 8)) || (rc = Q.keys_b.ensure((n_keys + 1) * 8)) || (rc = Q.rank_a.ensure((V + 1) * 8)) ||
        (rc = Q.rank_b.ensure((V + 1) * 8)) || (rc = Q.off.ensure((V + 1) * 8)) || (rc = Q.nbr.ensure((n_keys + 1) * 4)) ||
        (rc = Q.rank.ensure((V + 1) * 4)) || (rc = Q.order.ensure((V + 1) * 4)) || (rc = Q.kind.ensure(V + 1)) || (rc = Q.cnt_c.ensure((V + 1) * 8)) ||
        (rc = Q.cnt_e.ensure((V + 1) * 8)) || (rc = Q.counters.ensure(cl::kCounters * 8)) || (rc = Q.temp.ensure(temp_bytes ? temp_bytes : 16)))
        return rc;
    unsigned long long* d_counters = Q.counters.as<unsigned long long>();
    uint64_t *keys_a = Q.keys_a.as<uint64_t>(), *keys_b = Q.keys_b.as<uint64_t>(), *cnt_c = Q.cnt_c.as<uint64_t>(), *cnt_e = Q.cnt_e.as<uint64_t>();
    const cl::Graph view{g.edges_out.as<hc_edge_rec>(), g.out_off.as<unsigned long long>(), g.incl.as<uint8_t>(), (uint32_t)V, (uint32_t)E};
    const cl::Adj adj{Q.off.as<unsigned long long>(), Q.nbr.as<uint32_t>(), Q.rank.as<uint32_t>(), Q.order.as<uint32_t>(), Q.kind.as<uint8_t>(), (uint32_t)V, cap};
    float ms = 0;
    // 1. the pair set, the simple adjacency, the rank, the roots' kinds
    HC_HIP(hipMemsetAsync(d_counters, 0, cl::kCounters * 8, s));
    HC_HIP(hipMemsetAsync(d_counters + cl::kKey, 0xff, 8, s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(cl::emit_pairs(view, shift, keys_a, d_counters, s));
    if (n_keys) {
        HC_HIP(hc::prims::sort_keys(Q.temp.p, Q.temp.cap, keys_a, keys_b, n_keys, 0, (int)(2 * shift + 1), s));
        HC_HIP(hc::prims::unique(Q.temp.p, Q.temp.cap, keys_b, keys_a, d_counters + cl::kUnique, n_keys, s));
    }
    HC_HIP(cl::build_adjacency(keys_a, n_keys, shift, adj, Q.rank_a.as<uint64_t>(), d_counters, s));
    if (V) HC_HIP(hc::prims::sort_keys(Q.temp.p, Q.temp.cap, Q.rank_a.as<uint64_t>(), Q.rank_b.as<uint64_t>(), V, 0, 64, s));
    HC_HIP(cl::classify(Q.rank_b.as<uint64_t>(), adj, cnt_c, cnt_e, d_counters, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    unsigned long long h[cl::kCounters];
    uint64_t n_directed = 0;
    HC_HIP(hipMemcpyAsync(h, d_counters, sizeof h, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&n_directed, adj.off + V, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device = ms;
    if (h[cl::kKey] != hc::gtext::kNoKey) {  // the reference would have stopped here
        const uint64_t key = h[cl::kKey], place = (key >> 2) & 0x7fffffffull;
        counts->status = (key & 3) == 0 ? HC_CLIQUES_SELF_LOOP : HC_CLIQUES_INCLUSION_HAS_EDGES;
        counts->bad_v = key >> 33;
        counts->bad_pos = place ? place - 1 : 0;
        return HC_OK;
    }
    if (n_directed >= kLimit) return fail(HC_ERR_ARG, me + "2 * n_pairs is not below 2^31");
    counts->n_pairs = n_directed / 2;
    const uint64_t n_singletons = h[cl::kSingletons];  // (reported with the cliques: nothing kept, nothing counted)
    counts->n_host_roots = h[cl::kHostRoots];
    // 2. the count pass: scratch per resident wave, for the largest universe a wave can meet
    const uint32_t dmax = (uint32_t)(h[cl::kMaxDeg] < cap ? h[cl::kMaxDeg] : cap);
    const uint64_t slice = cl::slice_words(dmax);
    // (the walk waits on its own loads: the smaller the slice, the more waves a CU gets to hide that)
    const uint32_t n_waves = c->n_cu * 4u * (slice * 8 <= (8u << 10) ? 4u : slice * 8 <= (64u << 10) ? 2u : 1u);
    if (dmax) {
        if ((rc = Q.slices.ensure(slice * 8 * n_waves))) return rc;
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(cl::count_pass(adj, cnt_c, cnt_e, Q.slices.as<uint64_t>(), n_waves, dmax, budget, d_counters, s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(h, d_counters, sizeof h, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        counts->ms_device += ms;
    }
    bool over = h[cl::kOver] != 0;
    uint64_t biggest = h[cl::kMaxClique];
    if (n_singletons && biggest < 1) biggest = 1;
    // 3. the host's roots, from the fetched adjacency; their counts go in before the sums
    std::vector<HostRoot> host_roots;
    std::vector<uint64_t> h_c, h_e;
    if (!over && counts->n_host_roots) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint64_t> h_off(V + 1);
        std::vector<uint32_t> h_nbr(n_directed), h_rank(V), h_order(V);
        std::vector<uint8_t> h_kind(V);
        h_c.resize(V + 1), h_e.resize(V + 1);
        HC_HIP(hipMemcpyAsync(h_off.data(), adj.off, (V + 1) * 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_nbr.data(), adj.nbr, n_directed * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_rank.data(), adj.rank, V * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_order.data(), adj.order, V * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_kind.data(), adj.kind, V, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_c.data(), cnt_c, (V + 1) * 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_e.data(), cnt_e, (V + 1) * 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        for (uint64_t r = 0; r < V; r++)
            if (h_kind[r] == cl::kRootHost) {
                host_roots.emplace_back();
                host_roots.back().r = (uint32_t)r;
            }
        const cl::HostAdj ha{h_off.data(), h_nbr.data(), h_rank.data()};
        std::atomic<size_t> next{0};
        std::atomic<uint64_t> total{h[cl::kTotal] + n_singletons};
        std::atomic<bool> stop{false};
        auto work = [&]() {
            for (size_t k; !stop.load() && (k = next.fetch_add(1)) < host_roots.size();) {
                HostRoot& R = host_roots[k];
                const bool ok = cl::host_root(ha, h_order[R.r], budget, R.sizes, R.nodes, &R.entries, &R.biggest);
                if (!ok || total.fetch_add(R.entries) + R.entries > budget) stop.store(true);
            }
        };
        const uint32_t nt = st->n_threads ? st->n_threads : 1;
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < nt && t < host_roots.size(); t++) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
        over = stop.load();
        for (const HostRoot& R : host_roots) {
            h_c[R.r] = R.sizes.size(), h_e[R.r] = R.entries;
            biggest = R.biggest > biggest ? R.biggest : biggest;
        }
        if (!over) {
            HC_HIP(hipMemcpyAsync(cnt_c, h_c.data(), (V + 1) * 8, hipMemcpyHostToDevice, s));
            HC_HIP(hipMemcpyAsync(cnt_e, h_e.data(), (V + 1) * 8, hipMemcpyHostToDevice, s));
            HC_HIP(hipStreamSynchronize(s));  // (the copies have read h_c / h_e before they change)
            uint64_t sc = 0, se = 0;  // the sums the device is about to make, for the host roots' places
            for (uint64_t r = 0; r <= V; r++) {
                const uint64_t nc = h_c[r], ne = h_e[r];
                h_c[r] = sc, h_e[r] = se;
                sc += nc, se += ne;
            }
        }
        counts->ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (over) {
        counts->status = HC_CLIQUES_OVER_BUDGET;
        return HC_OK;
    }
    // 4. the sums: every root's first clique and first entry, the totals behind the last
    uint64_t n_cliques = 0, n_entries = 0;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, cnt_c, cnt_c, V + 1, s));
    HC_HIP(hc::prims::exclusive_sum(Q.temp.p, Q.temp.cap, cnt_e, cnt_e, V + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipMemcpyAsync(&n_cliques, cnt_c + V, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&n_entries, cnt_e + V, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device += ms;
    if (n_entries > budget) {  // (the count pass stops early only where it is sure; this is the verdict)
        counts->status = HC_CLIQUES_OVER_BUDGET;
        return HC_OK;
    }
    if (n_cliques >= kLimit || n_entries >= kLimit) return fail(HC_ERR_ARG, me + "n_cliques or n_entries is not below 2^31");
    // 5. the write pass
    if ((rc = Q.clique_off.ensure((n_cliques + 1) * 8)) || (rc = Q.clique_nodes.ensure((n_entries + 1) * 4))) return rc;
    unsigned long long* d_off = Q.clique_off.as<unsigned long long>();
    uint32_t* d_nodes = Q.clique_nodes.as<uint32_t>();
    HC_HIP(hipMemsetAsync(d_counters + cl::kTicket, 0, 8, s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(cl::write_pass(adj, cnt_c, cnt_e, Q.slices.as<uint64_t>(), n_waves, dmax, d_counters, d_off, d_nodes, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    std::vector<uint64_t> offs;
    if (!host_roots.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        for (const HostRoot& R : host_roots) {
            uint64_t at = h_e[R.r];
            for (uint32_t sz : R.sizes) offs.push_back(at), at += sz;
        }
        size_t k = 0;
        for (const HostRoot& R : host_roots) {  // (offs no longer grows: its addresses hold until the synchronize below)
            if (R.sizes.empty()) continue;
            HC_HIP(hipMemcpyAsync(d_off + h_c[R.r], offs.data() + k, R.sizes.size() * 8, hipMemcpyHostToDevice, s));
            HC_HIP(hipMemcpyAsync(d_nodes + h_e[R.r], R.nodes.data(), R.nodes.size() * 4, hipMemcpyHostToDevice, s));
            k += R.sizes.size();
        }
        HC_HIP(hipStreamSynchronize(s));
        counts->ms_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device += ms;
    counts->n_cliques = n_cliques;
    counts->n_singletons = n_singletons;
    counts->n_entries = n_entries;
    counts->max_clique = biggest;
    Q.n_cliques = n_cliques;
    Q.n_entries = n_entries;
    Q.valid = true;
    return HC_OK;
}

int hc_graph_cliques_fetch(hc_ctx* c, uint64_t* clique_off, uint32_t* clique_nodes) {
    if (!c) return fail(HC_ERR_ARG, "hc_graph_cliques_fetch: null context");
    const hc_ctx::Cliques& Q = c->cliques;
    if (!Q.valid) return fail(HC_ERR_STATE, "hc_graph_cliques_fetch: no cliques on the device (hc_graph_cliques first)");
    HC_HIP(hipSetDevice(c->device));
    if (clique_off) HC_HIP(hipMemcpyAsync(clique_off, Q.clique_off.p, (Q.n_cliques + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (clique_nodes && Q.n_entries) HC_HIP(hipMemcpyAsync(clique_nodes, Q.clique_nodes.p, Q.n_entries * 4, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

}  // extern "C"
