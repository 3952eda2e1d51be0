// hc_api_fno1_resident.cpp — hc_fno1_from_graph / hc_fno1_text_fetch / hc_fno1_edges_fetch / hc_fno1_lines_device (include/hcsr.h): FNO=1
// from the graph, the branching edges, the inclusion groups and (HC_FNO1_TABLES_KEPT) the tables the context keeps.  The edge list is built
// by hc_fno1_resident_kernels.hip around ordered selections, one exclusive sum and one stable radix sort (hc_prims.hip); from
// fno_clique_pairs on it is hc_fno1_run's own launch sequence (hc_api_fno.cpp: fno1_walk_from_device).  The list, the text and the lines
// are built in blocks of their own and trade places with the kept ones at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_fno1_resident.h"
#include "hc_fno_device.h"
#include "hc_prims.h"
#include "host/Types.h"

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

// The context's grow-only blocks behind the shared walk.  A block the walk gives back (hc_fno1_run frees it at that point) serves the next
// request it is large enough for — the smallest such block — so that the pool holds what is alive at once, not the sum of all requests;
// where none fits, the largest free block grows, and only then a new one is made.  Everything runs on one stream: a block's next user
// starts after its last one.
struct PoolAlloc final : hc::FnoAlloc {
    std::vector<hc_scratch>& pool;
    std::vector<uint8_t>& busy;
    PoolAlloc(std::vector<hc_scratch>& p, std::vector<uint8_t>& b) : pool(p), busy(b) { busy.assign(pool.size(), 0); }
    void* take(size_t bytes) override {
        bytes = bytes ? bytes : 16;
        size_t fit = pool.size(), largest = pool.size();
        for (size_t k = 0; k < pool.size(); k++) {
            if (busy[k]) continue;
            if (pool[k].cap >= bytes && (fit == pool.size() || pool[k].cap < pool[fit].cap)) fit = k;
            if (largest == pool.size() || pool[k].cap > pool[largest].cap) largest = k;
        }
        size_t k = fit != pool.size() ? fit : largest;
        if (k == pool.size()) {
            pool.emplace_back();
            busy.push_back(0);
        }
        if (pool[k].ensure(bytes) != HC_OK) throw hc::FatalError{HC_ERR_NOMEM, "find-next-overlaps on the device: hipMalloc failed"};
        busy[k] = 1;
        return pool[k].p;
    }
    void give_back(const void* p) override {  // (a block the pool does not own — the edge list, the kept tables — is left alone)
        for (size_t k = 0; p && k < pool.size(); k++)
            if (pool[k].p == p) busy[k] = 0;
    }
};

int bits_for(uint64_t n) {  // bits that hold every value below n (at least 1)
    int b = 1;
    while (b < 64 && ((n ? n - 1 : 0) >> b)) b++;
    return b;
}

}  // namespace

extern "C" {

int hc_fno1_from_graph(hc_ctx* c, const hc_fno1_resident_input* in, hc_fno1_resident_counts* counts) {
    namespace R = hc::fno1r;
    const char* me = "hc_fno1_from_graph";
    if (!c || !in || !counts) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    if (in->flags & ~HC_FNO_KNOWN_FLAGS) return fail(me, HC_ERR_ARG, "unknown bit in flags");
    if (in->flags & HC_FNO_ADD_DUPLICATES) return fail(me, HC_ERR_ARG, "HC_FNO_ADD_DUPLICATES: hc_fno1_run is the route for it");
    if (in->tables != HC_FNO1_TABLES_CALLER && in->tables != HC_FNO1_TABLES_KEPT) return fail(me, HC_ERR_ARG, "unknown value of tables");
    if (in->max_induced_pairs > R::kMaxCount) return fail(me, HC_ERR_ARG, "max_induced_pairs above 2^31 - 16");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(me, HC_ERR_STATE, "no graph on the device (hc_graph_resolve or hc_graph_load first)");
    const uint64_t V = g.n_vertices, G = g.n_edges, B = g.n_branching;
    const uint64_t n_groups = g.have_groups ? g.n_groups : 0;
    const bool kept_tables = in->tables == HC_FNO1_TABLES_KEPT;
    hc_ctx::SrMergeNext& M = c->sr_mn;
    uint64_t n_srs, new_read_count;
    if (kept_tables) {
        if (!M.tables_valid) return fail(me, HC_ERR_STATE, "no tables on the device (a successful hc_sr_merge_next or hc_sr_clique_next first)");
        if (M.tables_vertices != V) return fail(me, HC_ERR_STATE, "the kept tables are for another vertex count than the graph's");
        n_srs = M.tables_srs;
        new_read_count = M.tables_new_read_count;
    } else {
        n_srs = in->n_srs;
        new_read_count = in->new_read_count;
        if (in->n_nodes != V) return fail(me, HC_ERR_ARG, "n_nodes is not the graph's vertex count");
        if ((V && !in->nodes) || (n_srs && (!in->srs || !in->clique_off || !in->subread_off))) return fail(me, HC_ERR_ARG, "null array");
        for (uint64_t i = 1; i < n_srs; ++i)
            if (in->srs[i - 1].paired && !in->srs[i].paired)
                return fail(me, HC_ERR_ARG, "super-reads must be listed single-end first, then paired (single_SR_vec, paired_SR_vec)");
        for (uint64_t i = 0; i < n_srs; ++i)
            if (in->clique_off[i + 1] < in->clique_off[i] || in->subread_off[i + 1] < in->subread_off[i]) return fail(me, HC_ERR_ARG, "offsets descend");
        if (n_srs && ((in->clique_off[n_srs] && !in->clique_nodes) || (in->subread_off[n_srs] && !in->subreads))) return fail(me, HC_ERR_ARG, "null array");
    }
    const uint64_t N = (in->flags & HC_FNO_OPTIMIZE) ? 0 : in->n_nonedges;  // :926
    if (N && !in->nonedges) return fail(me, HC_ERR_ARG, "null array");
    const uint64_t max_pairs = in->max_induced_pairs ? in->max_induced_pairs : R::kMaxCount;
    counts->n_graph_edges = G;
    counts->n_branching = B;
    auto not_on_device = [&](const std::string& what) { return fail(me, HC_ERR_NOT_ON_DEVICE, what + ": hc_graph_fetch + hc_fno1_run decide"); };
    if (G + B + N >= R::kMaxCount || n_srs >= 0xFFFFFFFFull || V >= 0xFFFFFFFFull) return not_on_device("a count of 2^31 - 16 or more");
    const int id_bits = bits_for(new_read_count);
    if (new_read_count == 0 || 2 * id_bits > 62) return not_on_device("no new read, or ids that need more than 31 bits");

    hc_ctx::Fno1& F = c->fno1;
    F.ms_section[0] = F.ms_section[1] = F.ms_section[2] = F.ms_section[3] = 0;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    auto room = [&](hc_scratch& k, size_t bytes) { return k.ensure(bytes ? bytes : 16); };
    auto up = [&](hc_scratch& k, const void* p, size_t bytes) { return bytes ? hipMemcpyAsync(k.p, p, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    float ms = 0;
    double ms_device = 0;

    // the tables: uploaded once each, or read where hc_sr_merge_next / hc_sr_clique_next left them
    uint64_t clique_total = 0, sub_total = 0;
    const hc_fno_read *d_nodes, *d_srs;
    const uint64_t *d_clique_off, *d_clique_nodes, *d_sub_off;
    const hc_fno_subread* d_sub;
    if (kept_tables) {
        d_nodes = M.t_nodes.as<hc_fno_read>();
        d_srs = M.t_srs.as<hc_fno_read>();
        d_clique_off = M.t_clique_off.as<uint64_t>();
        d_clique_nodes = M.t_clique_nodes.as<uint64_t>();
        d_sub_off = M.t_sub_off.as<uint64_t>();
        d_sub = M.t_sub.as<hc_fno_subread>();
        if (n_srs) {
            HC_HIP(hipMemcpyAsync(&clique_total, d_clique_off + n_srs, 8, hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(&sub_total, d_sub_off + n_srs, 8, hipMemcpyDeviceToHost, s));
            HC_HIP(hipStreamSynchronize(s));
            if (clique_total * 8 > M.t_clique_nodes.cap || sub_total * sizeof(hc_fno_subread) > M.t_sub.cap)
                return fail(me, HC_ERR_STATE, "the kept tables' offsets leave their blocks");
        }
    } else {
        clique_total = n_srs ? in->clique_off[n_srs] : 0;
        sub_total = n_srs ? in->subread_off[n_srs] : 0;
        if ((rc = room(F.nodes, V * sizeof(hc_fno_read))) || (rc = room(F.srs, n_srs * sizeof(hc_fno_read))) || (rc = room(F.clique_off, (n_srs + 1) * 8)) ||
            (rc = room(F.clique_nodes, clique_total * 8)) || (rc = room(F.sub_off, (n_srs + 1) * 8)) || (rc = room(F.sub, sub_total * sizeof(hc_fno_subread))))
            return rc;
        HC_HIP(up(F.nodes, in->nodes, V * sizeof(hc_fno_read)));
        HC_HIP(up(F.srs, in->srs, n_srs * sizeof(hc_fno_read)));
        if (n_srs) {
            HC_HIP(up(F.clique_off, in->clique_off, (n_srs + 1) * 8));
            HC_HIP(up(F.sub_off, in->subread_off, (n_srs + 1) * 8));
        } else {
            HC_HIP(hipMemsetAsync(F.clique_off.p, 0, 8, s));
            HC_HIP(hipMemsetAsync(F.sub_off.p, 0, 8, s));
        }
        HC_HIP(up(F.clique_nodes, in->clique_nodes, clique_total * 8));
        HC_HIP(up(F.sub, in->subreads, sub_total * sizeof(hc_fno_subread)));
        d_nodes = F.nodes.as<hc_fno_read>();
        d_srs = F.srs.as<hc_fno_read>();
        d_clique_off = F.clique_off.as<uint64_t>();
        d_clique_nodes = F.clique_nodes.as<uint64_t>();
        d_sub_off = F.sub_off.as<uint64_t>();
        d_sub = F.sub.as<hc_fno_subread>();
    }
    if (clique_total >= R::kMaxCount || sub_total >= R::kMaxCount) return not_on_device("a count of 2^31 - 16 or more");

    // the pairs (i < j) in front of every inclusion group: one exclusive sum
    using hc::prims::scan_temp_bytes;
    using hc::prims::select_temp_bytes;
    using hc::prims::sort_temp_bytes;
    if ((rc = room(F.status, hc::kFnoCounters * 8)) || (rc = room(F.counts, R::kCounts * 8)) || (rc = room(F.pair_off, (n_groups + 1) * 8)) ||
        (rc = room(F.temp, scan_temp_bytes(n_groups + 1, 8))))
        return rc;
    unsigned long long* d_status = F.status.as<unsigned long long>();
    unsigned long long* d_counts = F.counts.as<unsigned long long>();
    uint64_t n_pairs = 0;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hipMemsetAsync(d_status, 0, hc::kFnoCounters * 8, s));
    HC_HIP(hipMemsetAsync(d_counts, 0, R::kCounts * 8, s));
    if (n_groups) {
        HC_HIP(R::group_pairs(g.incl_off.as<uint64_t>(), n_groups, F.pair_off.as<uint64_t>(), s));
        HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, F.pair_off.as<uint64_t>(), F.pair_off.as<uint64_t>(), n_groups + 1, s));
        HC_HIP(hipMemcpyAsync(&n_pairs, F.pair_off.as<uint64_t>() + n_groups, 8, hipMemcpyDeviceToHost, s));
    }
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    F.ms_section[0] = ms;
    counts->n_induced_pairs = n_pairs;
    counts->ms_device = ms_device;
    if (n_pairs > max_pairs) return not_on_device("more pairs inside the inclusion groups than max_induced_pairs");

    // segments 1 and 2, then checkEdge for the stored non-edges and the pairs: lanes, the long lists' waves, the ordered selections
    const uint64_t n_check = std::max(N, n_pairs);
    const size_t temp_bytes = std::max({select_temp_bytes(n_check ? n_check : 1), sort_temp_bytes(sub_total ? sub_total : 1, 8, 4)});
    if ((rc = room(F.next_edges, (G + B + N + std::min<uint64_t>(n_pairs, 1u << 16)) * sizeof(hc_fno_edge))) || (rc = room(F.nonedges, N * sizeof(hc_fno_edge))) ||
        (rc = room(F.keep, N + n_pairs)) || (rc = room(F.is_long, n_check)) || (rc = room(F.long_idx, n_check * 4)) ||
        (rc = room(F.sel_idx, (N + n_pairs) * 4)) || (rc = room(F.temp, temp_bytes)) || (rc = room(F.sub_sorted, sub_total * sizeof(hc_fno_subread))) ||
        (rc = room(F.sub_key_in, sub_total * 8)) || (rc = room(F.sub_key, sub_total * 8)) || (rc = room(F.sub_val_in, sub_total * 4)) ||
        (rc = room(F.sub_val, sub_total * 4)))
        return rc;
    hc_fno_edge* d_edges = F.next_edges.as<hc_fno_edge>();
    const R::Adj adj{d_edges, g.out_off.as<unsigned long long>(), d_nodes, V};
    const R::Groups groups{g.incl_edges.as<hc_edge_rec>(), g.incl_off.as<uint64_t>(), F.pair_off.as<uint64_t>(), n_groups, in->edge_threshold};
    uint8_t *keep_non = F.keep.as<uint8_t>(), *keep_ind = F.keep.as<uint8_t>() + N;
    uint32_t *sel_non = F.sel_idx.as<uint32_t>(), *sel_ind = F.sel_idx.as<uint32_t>() + N;
    HC_HIP(up(F.nonedges, in->nonedges, N * sizeof(hc_fno_edge)));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(R::convert(g.edges_out.as<hc_edge_rec>(), G, d_edges, s));
    HC_HIP(R::convert(g.branching.as<hc_edge_rec>(), B, d_edges + G, s));
    if (N) {
        HC_HIP(R::nonedge_lanes(F.nonedges.as<hc_fno_edge>(), N, adj, keep_non, F.is_long.as<uint8_t>(), d_status, s));
        HC_HIP(hc::prims::select_flagged(F.temp.p, F.temp.cap, F.is_long.as<uint8_t>(), N, F.long_idx.as<uint32_t>(), d_counts + R::kLongNon, s));
        HC_HIP(R::nonedge_waves(F.nonedges.as<hc_fno_edge>(), F.long_idx.as<uint32_t>(), d_counts + R::kLongNon, adj, keep_non, c->n_cu, s));
        HC_HIP(hc::prims::select_flagged(F.temp.p, F.temp.cap, keep_non, N, sel_non, d_counts + R::kKeptNon, s));
    }
    if (n_pairs) {
        HC_HIP(R::induced_lanes(groups, n_pairs, adj, keep_ind, F.is_long.as<uint8_t>(), d_status, s));
        HC_HIP(hc::prims::select_flagged(F.temp.p, F.temp.cap, F.is_long.as<uint8_t>(), n_pairs, F.long_idx.as<uint32_t>(), d_counts + R::kLongInd, s));
        HC_HIP(R::induced_waves(groups, F.long_idx.as<uint32_t>(), d_counts + R::kLongInd, adj, keep_ind, c->n_cu, s));
        HC_HIP(hc::prims::select_flagged(F.temp.p, F.temp.cap, keep_ind, n_pairs, sel_ind, d_counts + R::kKeptInd, s));
    }
    // the tables' checks and the subread maps in node order: one stable radix sort of super-read << 32 | node
    HC_HIP(R::cliques_check(d_clique_off, n_srs, d_status, s));
    if (sub_total) {
        HC_HIP(R::subread_keys(d_sub_off, d_sub, n_srs, sub_total, F.sub_key_in.as<uint64_t>(), F.sub_val_in.as<uint32_t>(), d_status, s));
        HC_HIP(hc::prims::sort_pairs(F.temp.p, F.temp.cap, F.sub_key_in.as<uint64_t>(), F.sub_key.as<uint64_t>(), F.sub_val_in.as<uint32_t>(),
                                     F.sub_val.as<uint32_t>(), sub_total, 0, 32 + bits_for(n_srs), s));
        HC_HIP(R::subread_gather(d_sub, F.sub_val.as<uint32_t>(), sub_total, F.sub_sorted.as<hc_fno_subread>(), s));
    }
    HC_HIP(hipEventRecord(c->ev1, s));
    unsigned long long h_status[hc::kFnoCounters], h_counts[R::kCounts];
    HC_HIP(hipMemcpyAsync(h_status, d_status, sizeof h_status, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(h_counts, d_counts, sizeof h_counts, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    F.ms_section[1] = ms;
    counts->ms_device = ms_device;
    if (h_status[4]) return not_on_device("a record the reference stops at, or a number outside what the device holds");
    const uint64_t kept = N ? h_counts[R::kKeptNon] : 0, I = n_pairs ? h_counts[R::kKeptInd] : 0, E = G + B + kept + I;
    if (kept > N || I > n_pairs) return fail(me, HC_ERR_STATE, "a selection kept more than it was given");
    counts->n_nonedges_kept = kept;
    counts->n_induced = I;
    if (E >= R::kMaxCount) return not_on_device("a count of 2^31 - 16 or more");
    // segments 3 and 4 behind the first two (the block grows, keeping them, where the survivors need more than it has)
    if (E * sizeof(hc_fno_edge) > F.next_edges.cap) {
        if ((rc = F.next_edges.grow_keep(E * sizeof(hc_fno_edge), (G + B) * sizeof(hc_fno_edge), s))) return rc;
        d_edges = F.next_edges.as<hc_fno_edge>();
    }
    const R::Adj adj_now{d_edges, adj.out_off, d_nodes, V};
    HC_HIP(hipEventRecord(c->ev0, s));
    if (kept) HC_HIP(hc::fno_gather_edges(F.nonedges.as<hc_fno_edge>(), sel_non, kept, d_edges + G + B, s));
    HC_HIP(R::induced_build(groups, sel_ind, I, adj_now, d_edges + G + B + kept, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    F.ms_section[2] = ms;
    counts->ms_device = ms_device;

    uint64_t walk_counters[5] = {0, 0, 0, 0, 0};
    hc::FnoTextSink sink;
    if (E) {
        hc::FnoWalkInput w{};
        w.edges = d_edges;
        w.n_edges = E;
        w.nodes = d_nodes;
        w.n_nodes = V;
        w.srs = d_srs;
        w.n_srs = n_srs;
        w.subread_off = d_sub_off;
        w.subreads = F.sub_sorted.as<hc_fno_subread>();
        w.new_read_count = new_read_count;
        w.id_bits = (uint32_t)id_bits;
        w.resolve_orientations = (in->flags & HC_FNO_RESOLVE_ORIENTATIONS) ? 1u : 0u;
        const hc::FnoWalkTables t{d_clique_off, d_clique_nodes, clique_total};
        sink.text_device = [&](uint64_t bytes) -> char* {
            if (F.next_text.ensure(bytes ? bytes : 16) != HC_OK) throw hc::FatalError{HC_ERR_NOMEM, "hipMalloc failed (the text)"};
            return F.next_text.as<char>();
        };
        sink.lines_device = [&](uint64_t n) -> hc_line_rec* {
            if (F.next_lines.ensure((n ? n : 1) * sizeof(hc_line_rec)) != HC_OK) throw hc::FatalError{HC_ERR_NOMEM, "hipMalloc failed (the lines)"};
            return F.next_lines.as<hc_line_rec>();
        };
        PoolAlloc pool(F.pool, F.pool_busy);
        bool ok = false;
        try {
            HC_HIP(hipEventRecord(c->ev0, s));
            ok = hc::fno1_walk_from_device(pool, s, w, t, (in->flags & HC_FNO_NO_INCLUSIONS) != 0, d_status, sink, walk_counters, nullptr,
                                           std::chrono::steady_clock::now());
            HC_HIP(hipEventRecord(c->ev1, s));
            HC_HIP(hipStreamSynchronize(s));
            HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            ms_device += ms;
            F.ms_section[3] = ms;
        } catch (const hc::FatalError& e) {
            return fail(me, e.status, e.what);
        }
        counts->ms_device = ms_device;
        counts->n_items = sink.n_items;
        if (!ok && sink.left != hc::kFnoLeftEmpty) return not_on_device("the walk met a record the reference stops at, or a number outside what the device holds");
        if (!ok) sink.n_bytes = 0, sink.n_items = 0, memset(walk_counters, 0, sizeof walk_counters);  // nothing to write
    }
    if ((rc = room(F.next_text, 0)) || (rc = room(F.next_lines, 0))) return rc;
    F.edges.swap(F.next_edges);
    F.text.swap(F.next_text);
    F.lines.swap(F.next_lines);
    F.n_seg[0] = G, F.n_seg[1] = B, F.n_seg[2] = kept, F.n_seg[3] = I;
    F.n_text = sink.n_bytes;
    F.n_lines = walk_counters[4];
    F.valid = true;
    counts->copied = walk_counters[0];
    counts->u2sr = walk_counters[1];
    counts->v2sr = walk_counters[2];
    counts->sr2sr = walk_counters[3];
    counts->n_lines = walk_counters[4];
    counts->n_bytes = sink.n_bytes;
    return HC_OK;
}

int hc_fno1_text_fetch(hc_ctx* c, uint64_t first, uint64_t count, char* dst) {
    const char* me = "hc_fno1_text_fetch";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    const hc_ctx::Fno1& F = c->fno1;
    if (!F.valid) return fail(me, HC_ERR_STATE, "no text on the device (hc_fno1_from_graph first)");
    if (first > F.n_text || count > F.n_text - first) return fail(me, HC_ERR_ARG, "range beyond the text");
    if (count == 0) return HC_OK;
    if (!dst) return fail(me, HC_ERR_ARG, "null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, F.text.as<char>() + first, count, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

int hc_fno1_edges_fetch(hc_ctx* c, uint64_t first, uint64_t count, hc_fno_edge* dst) {
    const char* me = "hc_fno1_edges_fetch";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    const hc_ctx::Fno1& F = c->fno1;
    if (!F.valid) return fail(me, HC_ERR_STATE, "no edge list on the device (hc_fno1_from_graph first)");
    const uint64_t n = F.n_seg[0] + F.n_seg[1] + F.n_seg[2] + F.n_seg[3];
    if (first > n || count > n - first) return fail(me, HC_ERR_ARG, "range beyond the list");
    if (count == 0) return HC_OK;
    if (!dst) return fail(me, HC_ERR_ARG, "null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, F.edges.as<hc_fno_edge>() + first, count * sizeof(hc_fno_edge), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

int hc_fno1_lines_device(hc_ctx* c, const hc_line_rec** d_lines, uint64_t* n_lines) {
    const char* me = "hc_fno1_lines_device";
    if (!c || !d_lines || !n_lines) return fail(me, HC_ERR_ARG, "null argument");
    const hc_ctx::Fno1& F = c->fno1;
    if (!F.valid) return fail(me, HC_ERR_STATE, "no lines on the device (hc_fno1_from_graph first)");
    *d_lines = F.lines.as<hc_line_rec>();
    *n_lines = F.n_lines;
    return HC_OK;
}

int hc_fno1_section_ms(hc_ctx* c, double ms[4]) {
    if (!c || !ms) return fail("hc_fno1_section_ms", HC_ERR_ARG, "null argument");
    for (int k = 0; k < 4; k++) ms[k] = c->fno1.ms_section[k];
    return HC_OK;
}

}  // extern "C"
