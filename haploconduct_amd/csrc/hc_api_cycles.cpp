// hc_api_cycles.cpp — hc_graph_sort_edges, hc_graph_remove_cycles and hc_graph_fetch_cycle_pairs (include/hcedge.h): the second
// OverlapGraph::sortEdges of an iteration and cycleRemovalHeuristic on the graph the context holds.  The sort's keys, radix sorts and
// in-list rebuild are hc_graph_kernels.hip's; the cycle kernels are hc_cycles_kernels.hip's; the walk is host/Cycles.cpp's; the edit is
// hc_br_reduce's (hc::graph_remove_records).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/hcedge.h"
#include "hc_ctx.h"
#include "hc_cycles.h"
#include "hc_graph.h"
#include "host/Cycles.h"
#include "host/Types.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {
namespace cy = hc::cycles;

static const char* const kTiedRefusal =
    ": the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first";

double ms_since(std::chrono::steady_clock::time_point& t0) {  // and the clock starts again
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
}

struct Carver {
    char* base;
    size_t at = 0;
    template <typename T>
    void take(T*& p, uint64_t n) {
        p = base ? (T*)(base + at) : nullptr;
        at += (n * sizeof(T) + 255) / 256 * 256;
    }
};

// the arrays of hc_graph_sort_edges in one block
struct SortWork {
    uint32_t *idx, *o_out, *o_in, *k32a, *k32b, *tmp_idx, *tied_list, *len;
    uint64_t *k64a, *k64b;
    uint8_t* tied;
};
size_t carve_sort(SortWork& w, char* base, uint64_t V, uint64_t E, uint64_t n_reads) {
    Carver c{base};
    c.take(w.idx, E), c.take(w.o_out, E), c.take(w.o_in, E), c.take(w.k32a, E), c.take(w.k32b, E), c.take(w.tmp_idx, E);
    c.take(w.k64a, E), c.take(w.k64b, E), c.take(w.tied, V + 1), c.take(w.tied_list, V + 1), c.take(w.len, n_reads + 1);
    return c.at;
}

// the per-graph arrays of cy::Work, and those of the compact CSR (n_sub_edges records, n_pairs pairs, n_table table entries)
size_t carve_graph(cy::Work& w, char* base, uint64_t V, uint64_t E) {
    Carver c{base};
    const uint64_t V1 = V + 1, E1 = E + 1;
    c.take(w.src, E1), c.take(w.tgt, E1), c.take(w.key, E1), c.take(w.col1, E1), c.take(w.rk_a, V1), c.take(w.rk_b, V1);
    c.take(w.parent, V1), c.take(w.root_flag, V1), c.take(w.vflag, V1), c.take(w.sub_vtx, V1), c.take(w.lid, V1), c.take(w.sub_off, V1 + 1);
    c.take(w.perm_base, V1), c.take(w.pair_u, E1), c.take(w.pairs, E1), c.take(w.rec, E1), c.take(w.in_pos, E1);
    return c.at;
}
size_t carve_sub(cy::Work& w, char* base, uint64_t n_sub_edges, uint64_t n_table) {
    Carver c{base};
    const uint64_t E1 = n_sub_edges + 1;
    c.take(w.sub_src, E1), c.take(w.sub_tgt, E1), c.take(w.sub_key, 3 * E1), c.take(w.cols, cy::kSubColumns * E1), c.take(w.table, n_table + 1);
    return c.at;
}

size_t carve_radix(cy::Work& w, char* base, uint64_t E) {
    Carver c{base};
    const uint64_t E1 = E + 1;
    c.take(w.rs_k32a, E1), c.take(w.rs_k32b, E1), c.take(w.rs_idx_a, E1), c.take(w.rs_idx_b, E1), c.take(w.rs_k64a, E1), c.take(w.rs_k64b, E1);
    return c.at;
}

hc::trans::Graph view_of(hc_ctx::Graph& g) {
    return hc::trans::Graph{g.edges_out.as<hc_edge_rec>(), g.o_out.as<uint32_t>(), g.out_off.as<unsigned long long>(), g.in_nodes.as<uint32_t>(),
                            g.in_off.as<unsigned long long>(), (uint32_t)g.n_vertices, (uint32_t)g.n_edges};
}
}  // namespace

extern "C" {

int hc_graph_sort_edges(hc_ctx* c, const uint32_t* len_by_read, uint64_t n_reads, hc_sort_counts* counts) {
    const std::string me = "hc_graph_sort_edges";
    if (!c || !counts || (n_reads && !len_by_read)) return fail(HC_ERR_ARG, me + ": null argument");
    memset(counts, 0, sizeof *counts);
    if (n_reads >= (1ull << 32)) return fail(HC_ERR_ARG, me + ": 2^32 reads and more");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, me + ": no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, me + kTiedRefusal);
    const uint64_t V = g.n_vertices, E = g.n_edges;
    counts->n_edges = E;
    if (E == 0) {  // nothing to order
        g.sorted_at = g.edits;
        return HC_OK;
    }
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    hc_ctx::Cycles& Q = c->cycles;
    SortWork w{};
    int rc;
    const size_t temp_bytes = std::max(hc::graph_temp_bytes((uint32_t)E, (uint32_t)(V ? V : 1)), cy::temp_bytes(E, V));
    if ((rc = Q.work.ensure(carve_sort(w, nullptr, V, E, n_reads))) || (rc = Q.temp.ensure(temp_bytes)) || (rc = Q.counters.ensure(cy::kCounters * 8)))
        return rc;
    carve_sort(w, Q.work.as<char>(), V, E, n_reads);
    unsigned long long* const d_counters = Q.counters.as<unsigned long long>();
    hc::trans::Graph in, out;
    if ((rc = hc::graph_clean_prepare(c, in, out))) return rc;
    // the current graph stays as it is until the commit: every kernel below writes scratch or the *_next buffers
    if (n_reads) HC_HIP(hipMemcpyAsync(w.len, len_by_read, n_reads * 4, hipMemcpyHostToDevice, s));
    HC_HIP(cy::sort_prepare(in, w.idx, n_reads, d_counters + cy::kBadRead, s));
    unsigned long long bad = 0;
    HC_HIP(hipMemcpyAsync(&bad, d_counters + cy::kBadRead, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    if (bad) return fail(HC_ERR_ARG, me + ": a record's read1 / read2 is not below n_reads");
    hc::GraphParams gp;
    gp.reads = nullptr;
    gp.n_reads = (uint32_t)n_reads;
    gp.vtx = nullptr;
    gp.n_vertices = (uint32_t)V;
    gp.ignore_inclusions = 0;
    gp.len_by_read = w.len;
    HC_HIP(hipMemsetAsync(w.tied, 0, V + 1, s));
    HC_HIP(hc::graph_orders(gp, in.edges, w.idx, (uint32_t)E, HC_GRAPH_SORTED, w.k32a, w.k32b, w.k64a, w.k64b, w.tmp_idx, w.o_out, w.o_in, out.out_off,
                            out.in_off, w.tied, Q.temp.p, Q.temp.cap, s));
    HC_HIP(hc::graph_gather(in.edges, w.o_out, w.o_in, (uint32_t)E, out.edges, out.in_nodes, s));
    HC_HIP(cy::gather_seq(in.seq, w.o_out, (uint32_t)E, out.seq, s));
    HC_HIP(hc::graph_select_tied(w.tied, (uint32_t)V, w.tied_list, d_counters + cy::kTied, Q.temp.p, Q.temp.cap, s));
    unsigned long long n_tied = 0;
    HC_HIP(hipMemcpyAsync(&n_tied, d_counters + cy::kTied, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    counts->n_tied_lists = n_tied;
    if (n_tied) {  // std::sort's own order of those lists, from their incoming order (the offsets are the same in both graphs)
        std::vector<uint32_t> tied(n_tied);
        std::vector<uint64_t> off(V + 1);
        HC_HIP(hipMemcpyAsync(tied.data(), w.tied_list, n_tied * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(off.data(), in.out_off, (V + 1) * 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        std::vector<hc_edge_rec> list;
        std::vector<uint32_t> seq;
        for (const uint32_t v : tied) {
            const uint64_t lo = off[v], n = off[v + 1] - lo;
            list.resize(n), seq.resize(n);
            HC_HIP(hipMemcpyAsync(list.data(), in.edges + lo, n * sizeof(hc_edge_rec), hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(seq.data(), in.seq + lo, n * 4, hipMemcpyDeviceToHost, s));
            HC_HIP(hipStreamSynchronize(s));
            cy::sort_out_list(list.data(), seq.data(), n, len_by_read);
            HC_HIP(hipMemcpyAsync(out.edges + lo, list.data(), n * sizeof(hc_edge_rec), hipMemcpyHostToDevice, s));
            HC_HIP(hipMemcpyAsync(out.seq + lo, seq.data(), n * 4, hipMemcpyHostToDevice, s));
            HC_HIP(hipStreamSynchronize(s));
        }
    }
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
    out.E = (uint32_t)E;
    hc::graph_clean_commit(c, out);
    g.sorted_at = g.edits;
    return HC_OK;
}

int hc_graph_remove_cycles(hc_ctx* c, const hc_cycles_settings* st, hc_cycles_counts* counts) {
    const std::string me = "hc_graph_remove_cycles";
    if (!c || !st || !counts) return fail(HC_ERR_ARG, me + ": null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::Graph& g = c->graph;
    hc_ctx::Cycles& Q = c->cycles;
    if (!g.valid) return fail(HC_ERR_STATE, me + ": no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, me + kTiedRefusal);
    counts->edges_before = counts->edges_after = g.n_edges;
    if (g.sorted_at != g.edits) {
        counts->status = HC_CYCLES_NOT_SORTED;
        return fail(HC_ERR_STATE, me + ": the graph is not in hc_graph_sort_edges' order (the call has not run, or the graph was edited since)");
    }
    Q.drop();
    const uint64_t V = g.n_vertices, E = g.n_edges;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    cy::Work w{};
    int rc;
    if ((rc = Q.work.ensure(carve_graph(w, nullptr, V, E))) || (rc = Q.temp.ensure(cy::temp_bytes(E, V))) || (rc = Q.counters.ensure(cy::kCounters * 8)) ||
        (rc = Q.pin.ensure((V + 1) * 16 + (E + 1) * 4)))
        return rc;
    carve_graph(w, Q.work.as<char>(), V, E);
    w.counters = Q.counters.as<unsigned long long>();
    w.temp = Q.temp.p, w.temp_bytes = Q.temp.cap;
    const hc::trans::Graph in = view_of(g);
    unsigned long long h[cy::kCounters];
    auto read_counters = [&]() -> hipError_t {
        const hipError_t e = hipMemcpyAsync(h, w.counters, sizeof h, hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };
    // try 1 over the whole graph: the roots' order and the target column come from the device, the host walks them
    uint64_t* const h_off = Q.pin.as<uint64_t>();
    uint64_t* const h_rk = h_off + V + 1;
    uint32_t* const h_col = (uint32_t*)(h_rk + V);
    auto clock = std::chrono::steady_clock::now();
    HC_HIP(cy::prepare(in, w, s));
    HC_HIP(read_counters());
    // a list longer than kRankMax: the columns by radix sorts instead of the ranking inside lists
    const bool radix = h[cy::kLongList] != 0;
    if (radix) {
        if ((rc = Q.work_radix.ensure(carve_radix(w, nullptr, E)))) return rc;
        carve_radix(w, Q.work_radix.as<char>(), E);
    }
    HC_HIP(cy::first_try(in, w, radix, s));
    HC_HIP(hipMemcpyAsync(h_off, in.out_off, (V + 1) * 8, hipMemcpyDeviceToHost, s));
    if (V) HC_HIP(hipMemcpyAsync(h_rk, w.rk_b, V * 8, hipMemcpyDeviceToHost, s));
    if (E) HC_HIP(hipMemcpyAsync(h_col, w.col1, E * 4, hipMemcpyDeviceToHost, s));
    HC_HIP(read_counters());
    counts->ms_first_device = ms_since(clock);
    std::vector<uint64_t> sets[cy::kTries];
    std::vector<uint32_t> roots(V);
    try {
        for (uint64_t i = 0; i < V; i++) roots[i] = (uint32_t)h_rk[i];
        cy::walk(roots.data(), V, h_off, h_col, (uint32_t)V, sets[0]);
    } catch (const std::bad_alloc&) {
        return fail(HC_ERR_NOMEM, me + ": out of memory");
    }
    counts->ms_first_walk = ms_since(clock);
    counts->tries = counts->best_try = 1;
    counts->try_size[0] = sets[0].size();
    if (sets[0].empty()) {  // :517: one try, nothing to report
        Q.valid = true;
        return HC_OK;
    }
    if (h[cy::kNanPlace] != cy::kNoPlace) {
        counts->status = HC_CYCLES_NAN_KEY;
        counts->bad_v = (uint32_t)(h[cy::kNanPlace] >> 32), counts->bad_pos = (uint32_t)h[cy::kNanPlace];
        return HC_OK;
    }
    // the components that own a pair, compacted: every other component is acyclic in every try
    const uint32_t n1 = (uint32_t)sets[0].size();
    std::vector<uint32_t> pair_u(n1);
    for (uint32_t k = 0; k < n1; k++) pair_u[k] = (uint32_t)(sets[0][k] >> 32);
    HC_HIP(hipMemcpyAsync(w.pair_u, pair_u.data(), (size_t)n1 * 4, hipMemcpyHostToDevice, s));
    HC_HIP(cy::components(in, w, n1, s));
    HC_HIP(read_counters());
    const uint32_t n_sub = (uint32_t)h[cy::kSubVertices];
    counts->n_flagged_components = h[cy::kComponents];
    HC_HIP(cy::compact(in, w, n_sub, s));
    std::vector<uint64_t> sub_off(n_sub + 1ull);
    std::vector<uint32_t> sub_vtx(n_sub);
    HC_HIP(hipMemcpyAsync(sub_off.data(), w.sub_off, (n_sub + 1ull) * 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(sub_vtx.data(), w.sub_vtx, (size_t)n_sub * 4, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    const uint64_t Es = sub_off[n_sub];
    counts->n_host_vertices = n_sub, counts->n_host_edges = Es;
    std::vector<uint32_t> sub_roots;
    try {
        // the permutation table: 16 rows per distinct list length
        std::map<uint32_t, uint64_t> base_of;
        std::vector<uint32_t> table;
        std::vector<uint64_t> perm_base(n_sub);
        for (uint32_t i = 0; i < n_sub; i++) {
            const uint32_t L = (uint32_t)(sub_off[i + 1] - sub_off[i]);
            auto it = base_of.find(L);
            if (it == base_of.end()) {
                it = base_of.emplace(L, table.size()).first;
                table.resize(table.size() + 16ull * L);
                cy::perm_table(L, table.data() + it->second);
            }
            perm_base[i] = it->second;
        }
        if ((rc = Q.work_sub.ensure(carve_sub(w, nullptr, Es, table.size()))) || (rc = Q.pin_sub.ensure((Es + 1) * 4 * cy::kSubColumns))) return rc;
        carve_sub(w, Q.work_sub.as<char>(), Es, table.size());
        if (!table.empty()) HC_HIP(hipMemcpyAsync(w.table, table.data(), table.size() * 4, hipMemcpyHostToDevice, s));
        if (n_sub) HC_HIP(hipMemcpyAsync(w.perm_base, perm_base.data(), (size_t)n_sub * 8, hipMemcpyHostToDevice, s));
        HC_HIP(cy::columns(in, w, n_sub, Es, radix, s));
        uint32_t* const h_cols = Q.pin_sub.as<uint32_t>();
        if (Es) HC_HIP(hipMemcpyAsync(h_cols, w.cols, Es * 4 * cy::kSubColumns, hipMemcpyDeviceToHost, s));  // one copy brings the columns back
        HC_HIP(hipStreamSynchronize(s));  // (also: the uploads have read `table` and `perm_base`)
        counts->ms_sub_device = ms_since(clock);
        // the roots of the compact CSR: the graph's order, which the ascending renumbering keeps
        std::vector<uint32_t> lid(V, 0xffffffffu);
        for (uint32_t i = 0; i < n_sub; i++) lid[sub_vtx[i]] = i;
        sub_roots.reserve(n_sub);
        for (uint64_t i = 0; i < V; i++)
            if (lid[roots[i]] != 0xffffffffu) sub_roots.push_back(lid[roots[i]]);
        const uint32_t* col_ptr[cy::kSubColumns];
        for (uint32_t t = 0; t < cy::kSubColumns; t++) col_ptr[t] = h_cols + t * Es;
        cy::walk_tries(sub_roots.data(), n_sub, sub_off.data(), col_ptr, n_sub, 2, cy::kTries, c->settings.n_threads ? c->settings.n_threads : 1, sets + 1);
        for (uint32_t t = 1; t < cy::kTries; t++)
            for (uint64_t& p : sets[t]) p = (uint64_t)sub_vtx[p >> 32] << 32 | sub_vtx[(uint32_t)p];
    } catch (const hc::FatalError& e) {
        return fail(e.status, me + ": " + e.what);
    } catch (const std::bad_alloc&) {
        return fail(HC_ERR_NOMEM, me + ": out of memory");
    }
    counts->ms_sub_walk = ms_since(clock);
    // a try's total: try 1's pairs in the unflagged components (none) plus its walk of the compact CSR
    counts->tries = cy::kTries;
    uint32_t best = 0;
    for (uint32_t t = 0; t < cy::kTries; t++) {
        counts->try_size[t] = sets[t].size();
        if (sets[t].size() < sets[best].size()) best = t;  // :522: strictly smaller
    }
    counts->best_try = best + 1;
    counts->backedge_count = sets[best].size();
    Q.pairs = sets[best];
    Q.valid = true;
    if (!st->remove_edges) return HC_OK;
    const uint32_t n = (uint32_t)Q.pairs.size();
    HC_HIP(hipMemcpyAsync(w.pairs, Q.pairs.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    HC_HIP(cy::find_records(in, w, n, s));
    HC_HIP(read_counters());
    if (h[cy::kMissing]) return fail(HC_ERR_STATE, me + ": removeEdge: Edge to be removed not found");
    // from here on the lists are replaced: the records leave in (u, v) order and follow branching_edges
    if ((rc = hc::graph_remove_records(c, me.c_str(), w.rec, w.in_pos, n, nullptr, 0))) return rc;
    g.sorted_at = g.edits;  // (what remains keeps its order)
    counts->edges_after = g.n_edges;
    counts->ms_edit = ms_since(clock);
    return HC_OK;
}

int hc_graph_fetch_cycle_pairs(hc_ctx* c, uint32_t* pairs, uint64_t cap, uint64_t* n_pairs) {
    if (!c || !n_pairs) return fail(HC_ERR_ARG, "hc_graph_fetch_cycle_pairs: null argument");
    *n_pairs = 0;
    const hc_ctx::Cycles& Q = c->cycles;
    if (!c->graph.valid || !Q.valid) return fail(HC_ERR_STATE, "hc_graph_fetch_cycle_pairs: no pairs kept (hc_graph_remove_cycles first)");
    *n_pairs = Q.pairs.size();
    for (uint64_t k = 0; pairs && k < Q.pairs.size() && k < cap; k++) pairs[2 * k] = (uint32_t)(Q.pairs[k] >> 32), pairs[2 * k + 1] = (uint32_t)Q.pairs[k];
    return HC_OK;
}

}  // extern "C"
