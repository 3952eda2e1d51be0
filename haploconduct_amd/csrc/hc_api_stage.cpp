// hc_api_stage.cpp — what the stage (construct_edges) needs of the device beyond plain scoring (include/hcedge.h):
//   hc_block_*  : one block of candidates in flight — H2D of the compact records, the scoring kernel appending the
//                 non-dropped records straight into page-locked host memory, one event to wait on;
//   hc_graph_*  : duplicate resolution + adjacency lists on the device (kernels: hc_graph_kernels.hip), and the
//                 cleaning of that graph: removeInclusions + removeTransitiveEdges (kernels: hc_trans_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/hcedge.h"
#include "hc_ctx.h"
#include "hc_graph.h"
#include "hc_trans.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

struct hc_block {
    hc_ctx* ctx = nullptr;
    uint64_t cap = 0;  // candidates
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hc_scratch d_in;                             // cap hc_cand_rec
    hc_scratch d_out;                            // cap hc_result_rec
    hc_scratch d_count;                          // unsigned long long: rows appended by the kernel
    hc_scratch d_rows;                           // cap hc_gather_row: the non-dropped records in sequence order (launch_kept_rows)
    hc_scratch d_tiles;                          // its scratch: two arrays of cap / 1024 + 2 uint32 counters
    hc_scratch h_rows{hipHostMallocMapped};      // page-locked, mapped: the rows, streamed out by a copy kernel behind it
    hc_scratch h_count{hipHostMallocDefault};    // page-locked: unsigned long long
    uint64_t n = 0, base_index = 0;
    hc_bucket_ws bucket;                   // scratch of a length-bucketed scoring launch (read sets of mixed sequence length)
    bool in_flight = false;
};

extern "C" {

int hc_block_create(hc_ctx* c, uint64_t max_candidates, hc_block** out) {
    if (!c || !out || max_candidates == 0 || max_candidates >= (1ull << 31)) return fail(HC_ERR_ARG, "hc_block_create: bad argument");
    *out = nullptr;
    HC_HIP(hipSetDevice(c->device));
    hc_block* b = new (std::nothrow) hc_block();
    if (!b) return fail(HC_ERR_NOMEM, "hc_block_create: host allocation failed");
    b->ctx = c;
    b->cap = max_candidates;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&b->done, hipEventDisableTiming)) != hipSuccess ||
        (e = b->d_in.alloc(max_candidates * sizeof(hc_cand_rec))) != hipSuccess ||
        (e = b->d_out.alloc(max_candidates * sizeof(hc_result_rec))) != hipSuccess ||
        (e = b->d_count.alloc(sizeof(unsigned long long))) != hipSuccess ||
        (e = b->d_rows.alloc(max_candidates * sizeof(hc_gather_row))) != hipSuccess ||
        (e = b->d_tiles.alloc(2 * (max_candidates / 1024 + 2) * sizeof(uint32_t))) != hipSuccess ||
        (e = b->h_rows.alloc(max_candidates * sizeof(hc_gather_row))) != hipSuccess ||
        (e = b->h_count.alloc(sizeof(unsigned long long))) != hipSuccess) {
        hc_block_destroy(b);
        return fail(HC_ERR_HIP, std::string("hc_block_create: ") + hipGetErrorString(e));
    }
    *out = b;
    return HC_OK;
}

int hc_block_destroy(hc_block* b) {
    if (!b) return HC_OK;
    (void)hipSetDevice(b->ctx->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->done) (void)hipEventDestroy(b->done);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
    return HC_OK;
}

int hc_block_submit(hc_block* b, const hc_cand_rec* cands, uint64_t n, uint64_t base_index) {
    if (!b) return fail(HC_ERR_ARG, "hc_block_submit: null block");
    hc_ctx* c = b->ctx;
    if (!c->have_reads) return fail(HC_ERR_STATE, "hc_block_submit: hc_set_reads has not been called");
    if (b->in_flight) return fail(HC_ERR_STATE, "hc_block_submit: the block is still in flight (hc_block_wait first)");
    if (n > b->cap) return fail(HC_ERR_ARG, "hc_block_submit: more candidates than the block was created for");
    if (n && !cands) return fail(HC_ERR_ARG, "hc_block_submit: null records");
    HC_HIP(hipSetDevice(c->device));
    b->n = n;
    b->base_index = base_index;
    *b->h_count.as<unsigned long long>() = 0;
    if (n) {
        void* d_rows = nullptr;
        uint32_t* const d_tiles = b->d_tiles.as<uint32_t>();
        unsigned long long* const d_count = b->d_count.as<unsigned long long>();
        HC_HIP(hipHostGetDevicePointer(&d_rows, b->h_rows.p, 0));
        HC_HIP(hipMemcpyAsync(b->d_in.p, cands, n * sizeof(hc_cand_rec), hipMemcpyHostToDevice, b->stream));
        // as given: the stage's blocks come from files in sfo2overlaps / FNO order; an unordered file still scores
        // correctly, only slower (hc_set_reorder(HC_REORDER_ALWAYS) sorts every block first)
        int rc = hc_ctx_score(c, HC_REC_COMPACT, b->d_in.p, n, b->d_out.p, b->stream, false, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, &b->bucket);
        if (rc) return rc;
        HC_HIP(hc::launch_kept_rows(b->d_out.as<hc_result_rec>(), n, nullptr, base_index, d_tiles, d_tiles + (b->cap / 1024 + 2),
                                    b->d_rows.as<hc_gather_row>(), b->cap, d_count, nullptr, nullptr, b->stream));
        HC_HIP(hc::launch_flush_rows(b->d_rows.p, d_rows, d_count, b->cap, sizeof(hc_gather_row), c->n_cu, b->stream));
        HC_HIP(hipMemcpyAsync(b->h_count.p, d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
    }
    HC_HIP(hipEventRecord(b->done, b->stream));
    b->in_flight = true;
    return HC_OK;
}

int hc_block_wait(hc_block* b, const hc_gather_row** rows, uint64_t* n_rows) {
    if (!b || !rows || !n_rows) return fail(HC_ERR_ARG, "hc_block_wait: null argument");
    *rows = nullptr;
    *n_rows = 0;
    if (!b->in_flight) return fail(HC_ERR_STATE, "hc_block_wait: nothing was submitted");
    HC_HIP(hipSetDevice(b->ctx->device));
    HC_HIP(hipEventSynchronize(b->done));
    b->in_flight = false;
    const uint64_t k = *b->h_count.as<unsigned long long>();
    if (k > b->cap) return fail(HC_ERR_STATE, "hc_block_wait: row count beyond the block's capacity");
    *rows = b->h_rows.as<hc_gather_row>();  // in sequence order as they are (launch_kept_rows)
    *n_rows = k;
    return HC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
int hc_graph_begin(hc_ctx* c) {
    if (!c) return fail(HC_ERR_ARG, "hc_graph_begin: null context");
    c->graph.n_appended = 0;
    c->graph.valid = false;
    c->graph.have_groups = false;
    return HC_OK;
}

int hc_graph_append(hc_ctx* c, const hc_admit_rec* admitted, uint64_t n) {
    if (!c || (n && !admitted)) return fail(HC_ERR_ARG, "hc_graph_append: null argument");
    if (n == 0) return HC_OK;
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::Graph& g = c->graph;
    g.valid = false;
    const uint64_t have = g.n_appended, want = have + n;
    if (want >= (1ull << 31)) return fail(HC_ERR_ARG, "hc_graph_append: more than 2^31-1 records");
    if (want * sizeof(hc_admit_rec) > g.adm.cap) {  // grow, keeping what is there
        size_t cap = g.adm.cap ? g.adm.cap : ((size_t)1 << 24);
        while (cap < want * sizeof(hc_admit_rec)) cap *= 2;
        if (const int rc = g.adm.grow_keep(cap, have * sizeof(hc_admit_rec), c->stream)) return rc;  // (appends in flight land in the old buffer first)
    }
    // through a page-locked buffer, asynchronously on the context's stream (the blocks score on their own streams;
    // hc_graph_resolve runs on this one, behind the copies): the caller — the stage's in-order half — does not wait
    const int t = g.stage_turn;
    g.stage_turn ^= 1;
    const size_t bytes = n * sizeof(hc_admit_rec);
    if (!g.stage_free[t]) HC_HIP(hipEventCreateWithFlags(&g.stage_free[t], hipEventDisableTiming));
    else HC_HIP(hipEventSynchronize(g.stage_free[t]));  // its previous copy (two appends ago) has left the buffer
    if (g.h_stage[t].cap < bytes) {
        size_t cap = (size_t)1 << 20;
        while (cap < bytes) cap *= 2;
        if (const int rc = g.h_stage[t].ensure_exact(cap)) return rc;
    }
    memcpy(g.h_stage[t].p, admitted, bytes);
    HC_HIP(hipMemcpyAsync((char*)g.adm.p + have * sizeof(hc_admit_rec), g.h_stage[t].p, bytes, hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipEventRecord(g.stage_free[t], c->stream));
    g.n_appended = want;
    return HC_OK;
}

int hc_graph_resolve(hc_ctx* c, const hc_admit_rec* admitted, uint64_t n, uint64_t n_vertices, const uint32_t* vertex_of_read,
                     uint32_t order, hc_graph_counts* counts) {
    if (!c || !counts) return fail(HC_ERR_ARG, "hc_graph_resolve: null argument");
    memset(counts, 0, sizeof *counts);
    counts->first_bad = -1;
    if (!c->have_reads) return fail(HC_ERR_STATE, "hc_graph_resolve: hc_set_reads has not been called");
    const bool appended = admitted == nullptr && n != 0;
    if (appended && n != c->graph.n_appended) return fail(HC_ERR_ARG, "hc_graph_resolve: n differs from the number of appended records");
    if (order != HC_GRAPH_INSERTION_ORDER && order != HC_GRAPH_SORTED) return fail(HC_ERR_ARG, "hc_graph_resolve: unknown order");
    if (n >= (1ull << 31) || n_vertices >= (1ull << 31)) return fail(HC_ERR_ARG, "hc_graph_resolve: more than 2^31-1 records or vertices");
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::Graph& g = c->graph;
    g.valid = false;
    g.have_groups = false;
    g.n_branching = g.n_tip_reads = 0;
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop(), c->label.drop();  // (hc_graph_write_text's text was the old graph's)
    c->br.drop();          // (and hc_br_evidence's tables)
    g.sorted_at = ~0ull, c->cycles.drop();  // (and hc_graph_sort_edges' stamp, hc_graph_remove_cycles' pairs)
    const uint32_t m = (uint32_t)n, V = (uint32_t)n_vertices;
    hipStream_t s = c->stream;
    const size_t m1 = m ? m : 1;
    int rc;
#define ENS(buf, bytes)                                 \
    if ((rc = g.buf.ensure(bytes)) != HC_OK) return rc
    if (!appended) ENS(adm, m1 * sizeof(hc_admit_rec));
    ENS(E, m1 * sizeof(hc_edge_rec));
    ENS(key0, m1 * 8);
    ENS(key1, m1 * 8);
    ENS(idx0, m1 * 4);
    ENS(idx1, m1 * 4);
    ENS(keep, m1);
    ENS(incl, (size_t)V + 1);
    ENS(tied, (size_t)V + 1);
    ENS(counters, 8 * sizeof(unsigned long long));
    ENS(surv, m1 * 4);
    ENS(k32a, m1 * 4);
    ENS(k32b, m1 * 4);
    ENS(k64a, m1 * 8);
    ENS(k64b, m1 * 8);
    ENS(tmp_idx, m1 * 4);
    ENS(o_out, m1 * 4);
    ENS(o_in, m1 * 4);
    ENS(out_off, ((size_t)V + 1) * 8);
    ENS(in_off, ((size_t)V + 1) * 8);
    ENS(in_nodes, m1 * 4);
    ENS(tied_list, ((size_t)V + 1) * 4);
    ENS(temp, hc::graph_temp_bytes(m ? m : 1, V ? V : 1));
    hc::GraphParams gp;
    gp.reads = c->d_reads.as<hc::ReadDesc>();
    gp.n_reads = c->view.n_reads;
    gp.vtx = nullptr;
    gp.n_vertices = V;
    gp.ignore_inclusions = (c->settings.flags & HC_FLAG_IGNORE_INCLUSIONS) ? 1u : 0u;
    if (vertex_of_read) {
        ENS(vtx, (size_t)(c->view.n_reads ? c->view.n_reads : 1) * 4);
        HC_HIP(hipMemcpyAsync(g.vtx.p, vertex_of_read, (size_t)c->view.n_reads * 4, hipMemcpyHostToDevice, s));
        gp.vtx = g.vtx.as<uint32_t>();
    }
    unsigned long long init[8] = {0, 0, 0, 0, ~0ull, 0, 0, 0};
    HC_HIP(hipMemcpyAsync(g.counters.p, init, sizeof init, hipMemcpyHostToDevice, s));
    HC_HIP(hipMemsetAsync(g.keep.p, 0, m1, s));
    HC_HIP(hipMemsetAsync(g.incl.p, 0, (size_t)V + 1, s));
    HC_HIP(hipMemsetAsync(g.tied.p, 0, (size_t)V + 1, s));
    unsigned long long* d_count = g.counters.as<unsigned long long>() + 5;
    if (m) {
        if (!appended) {
            HC_HIP(hipMemcpyAsync(g.adm.p, admitted, (size_t)m * sizeof(hc_admit_rec), hipMemcpyHostToDevice, s));
            g.n_appended = 0;
        }
        HC_HIP(hc::graph_build_and_replay(gp, g.adm.as<hc_admit_rec>(), m, g.E.as<hc_edge_rec>(), g.key0.as<uint64_t>(), g.key1.as<uint64_t>(),
                                          g.idx0.as<uint32_t>(), g.idx1.as<uint32_t>(), g.keep.as<uint8_t>(), g.incl.as<uint8_t>(),
                                          g.counters.as<unsigned long long>(), g.surv.as<uint32_t>(), d_count, g.temp.p, g.temp.cap, s));
    }
    unsigned long long h[8];
    HC_HIP(hipMemcpyAsync(h, g.counters.p, sizeof h, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    const uint32_t n_edges = m ? (uint32_t)h[5] : 0u;
    counts->n_admitted = m;
    counts->n_edges = n_edges;
    counts->inclusion_count = h[0];
    counts->dup_count = h[1];
    counts->first_bad = h[4] == ~0ull ? -1 : (int64_t)h[4];
    if (counts->first_bad >= 0) return HC_OK;  // the caller reports it; nothing to fetch
    if (m && h[2] != n_edges) return fail(HC_ERR_STATE, "hc_graph_resolve: slots and survivors disagree");
    ENS(edges_out, (size_t)(n_edges ? n_edges : 1) * sizeof(hc_edge_rec));
    HC_HIP(hc::graph_orders(gp, g.E.as<hc_edge_rec>(), g.surv.as<uint32_t>(), n_edges, order, g.k32a.as<uint32_t>(), g.k32b.as<uint32_t>(),
                            g.k64a.as<uint64_t>(), g.k64b.as<uint64_t>(), g.tmp_idx.as<uint32_t>(), g.o_out.as<uint32_t>(), g.o_in.as<uint32_t>(),
                            g.out_off.as<unsigned long long>(), g.in_off.as<unsigned long long>(), g.tied.as<uint8_t>(), g.temp.p, g.temp.cap, s));
    HC_HIP(hc::graph_gather(g.E.as<hc_edge_rec>(), g.o_out.as<uint32_t>(), g.o_in.as<uint32_t>(), n_edges, g.edges_out.as<hc_edge_rec>(),
                            g.in_nodes.as<uint32_t>(), s));
    uint64_t n_tied = 0;
    if (order == HC_GRAPH_SORTED && n_edges && V) {
        unsigned long long* d_tied_count = g.counters.as<unsigned long long>() + 6;
        HC_HIP(hc::graph_select_tied(g.tied.as<uint8_t>(), V, g.tied_list.as<uint32_t>(), d_tied_count, g.temp.p, g.temp.cap, s));
        unsigned long long t = 0;
        HC_HIP(hipMemcpyAsync(&t, d_tied_count, sizeof t, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        n_tied = t;
    }
#undef ENS
    counts->n_tied_lists = n_tied;
    g.n_vertices = V;
    g.n_edges = n_edges;
    g.n_tied = n_tied;
    g.valid = true;
    return HC_OK;
}

int hc_graph_fetch(hc_ctx* c, hc_edge_rec* edges, uint64_t* out_off, uint32_t* in_nodes, uint64_t* in_off, uint32_t* seq, uint8_t* inclusions,
                   uint32_t* tied_vertices) {
    if (!c) return fail(HC_ERR_ARG, "hc_graph_fetch: null context");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_fetch: no resolved graph on the device");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t E = g.n_edges, V = g.n_vertices;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are copied as they are");
    if (edges && E) HC_HIP(hipMemcpyAsync(edges, g.edges_out.p, E * sizeof(hc_edge_rec), hipMemcpyDeviceToHost, s));
    if (out_off) HC_HIP(hipMemcpyAsync(out_off, g.out_off.p, (V + 1) * 8, hipMemcpyDeviceToHost, s));
    if (in_nodes && E) HC_HIP(hipMemcpyAsync(in_nodes, g.in_nodes.p, E * 4, hipMemcpyDeviceToHost, s));
    if (in_off) HC_HIP(hipMemcpyAsync(in_off, g.in_off.p, (V + 1) * 8, hipMemcpyDeviceToHost, s));
    if (seq && E) HC_HIP(hipMemcpyAsync(seq, g.o_out.p, E * 4, hipMemcpyDeviceToHost, s));
    if (inclusions && V) HC_HIP(hipMemcpyAsync(inclusions, g.incl.p, V, hipMemcpyDeviceToHost, s));
    if (tied_vertices && g.n_tied) HC_HIP(hipMemcpyAsync(tied_vertices, g.tied_list.p, g.n_tied * 4, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    return HC_OK;
}

int hc_graph_fetch_edges(hc_ctx* c, uint64_t first, uint64_t count, hc_edge_rec* dst) {
    if (!c) return fail(HC_ERR_ARG, "hc_graph_fetch_edges: null context");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_fetch_edges: no resolved graph on the device");
    if (first > g.n_edges || count > g.n_edges - first) return fail(HC_ERR_ARG, "hc_graph_fetch_edges: range beyond the edges");
    if (count == 0) return HC_OK;
    if (!dst) return fail(HC_ERR_ARG, "hc_graph_fetch_edges: null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, g.edges_out.as<hc_edge_rec>() + first, count * sizeof(hc_edge_rec), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// graph cleaning

int hc_graph_size(hc_ctx* c, uint64_t* n_vertices, uint64_t* n_edges) {
    if (!c || !n_vertices || !n_edges) return fail(HC_ERR_ARG, "hc_graph_size: null argument");
    if (!c->graph.valid) return fail(HC_ERR_STATE, "hc_graph_size: no graph on the device");
    *n_vertices = c->graph.n_vertices;
    *n_edges = c->graph.n_edges;
    return HC_OK;
}

int hc_graph_load(hc_ctx* c, const hc_edge_rec* edges, const uint64_t* out_off, const uint32_t* in_nodes, const uint64_t* in_off,
                  uint64_t n_vertices, uint64_t n_edges, const uint8_t* inclusions) {
    if (!c || !out_off || !in_off || (n_edges && (!edges || !in_nodes))) return fail(HC_ERR_ARG, "hc_graph_load: null argument");
    if (n_edges >= (1ull << 31) || n_vertices >= (1ull << 31)) return fail(HC_ERR_ARG, "hc_graph_load: more than 2^31-1 edges or vertices");
    // the kernels index by these ids: the offsets are checked here (O(V)), the records and in-lists on the device after the copy
    const uint64_t V = n_vertices, E = n_edges;
    if (out_off[0] != 0 || in_off[0] != 0 || out_off[V] != E || in_off[V] != E) return fail(HC_ERR_ARG, "hc_graph_load: offsets do not span the edges");
    for (uint64_t v = 0; v < V; v++)
        if (out_off[v + 1] < out_off[v] || in_off[v + 1] < in_off[v]) return fail(HC_ERR_ARG, "hc_graph_load: offsets decrease");
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::Graph& g = c->graph;
    g.valid = false;
    g.have_groups = false;
    g.n_branching = g.n_tip_reads = 0;
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop(), c->label.drop();  // (hc_graph_write_text's text was the old graph's)
    c->br.drop();          // (and hc_br_evidence's tables)
    g.sorted_at = ~0ull, c->cycles.drop();  // (and hc_graph_sort_edges' stamp, hc_graph_remove_cycles' pairs)
    int rc;
    const size_t E1 = E ? E : 1;
    if ((rc = g.edges_out.ensure(E1 * sizeof(hc_edge_rec))) || (rc = g.o_out.ensure(E1 * 4)) || (rc = g.in_nodes.ensure(E1 * 4)) ||
        (rc = g.out_off.ensure((V + 1) * 8)) || (rc = g.in_off.ensure((V + 1) * 8)) || (rc = g.incl.ensure(V + 1)) ||
        (rc = g.clean_temp.ensure(hc::trans::temp_bytes(E, V))))
        return rc;
    hipStream_t s = c->stream;
    if (E) {
        HC_HIP(hipMemcpyAsync(g.edges_out.p, edges, E * sizeof(hc_edge_rec), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(g.in_nodes.p, in_nodes, E * 4, hipMemcpyHostToDevice, s));
    }
    HC_HIP(hipMemcpyAsync(g.out_off.p, out_off, (V + 1) * 8, hipMemcpyHostToDevice, s));
    HC_HIP(hipMemcpyAsync(g.in_off.p, in_off, (V + 1) * 8, hipMemcpyHostToDevice, s));
    HC_HIP(hipMemsetAsync(g.incl.p, 0, V + 1, s));
    if (inclusions && V) HC_HIP(hipMemcpyAsync(g.incl.p, inclusions, V, hipMemcpyHostToDevice, s));
    const hc::trans::Graph view{g.edges_out.as<hc_edge_rec>(), g.o_out.as<uint32_t>(), g.out_off.as<unsigned long long>(), g.in_nodes.as<uint32_t>(),
                                g.in_off.as<unsigned long long>(), (uint32_t)V, (uint32_t)E};
    bool consistent = false;
    HC_HIP(hc::trans::check_graph(view, &consistent, g.clean_temp.p, g.clean_temp.cap, s));
    if (!consistent)
        return fail(HC_ERR_ARG, "hc_graph_load: an edge lies in the wrong list or leaves the graph, or adj_in and adj_out hold different pairs");
    g.n_vertices = V;
    g.n_edges = E;
    g.n_tied = 0;
    g.valid = true;
    return HC_OK;
}

// the *_next buffers for a graph of (at most) E edges and V vertices, the scratch, and the views of both graphs
static int clean_prepare(hc_ctx* c, hc::trans::Graph& in, hc::trans::Graph& out) {
    hc_ctx::Graph& g = c->graph;
    const uint64_t E = g.n_edges, V = g.n_vertices, E1 = E ? E : 1;
    int rc;
    if ((rc = g.edges_next.ensure(E1 * sizeof(hc_edge_rec))) || (rc = g.seq_next.ensure(E1 * 4)) || (rc = g.in_nodes_next.ensure(E1 * 4)) ||
        (rc = g.out_off_next.ensure((V + 1) * 8)) || (rc = g.in_off_next.ensure((V + 1) * 8)) ||
        (rc = g.clean_temp.ensure(hc::trans::temp_bytes(E, V))))
        return rc;
    in = hc::trans::Graph{g.edges_out.as<hc_edge_rec>(), g.o_out.as<uint32_t>(), g.out_off.as<unsigned long long>(), g.in_nodes.as<uint32_t>(),
                          g.in_off.as<unsigned long long>(), (uint32_t)V, (uint32_t)E};
    out = hc::trans::Graph{g.edges_next.as<hc_edge_rec>(), g.seq_next.as<uint32_t>(), g.out_off_next.as<unsigned long long>(),
                           g.in_nodes_next.as<uint32_t>(), g.in_off_next.as<unsigned long long>(), (uint32_t)V, 0};
    return HC_OK;
}

static void clean_commit(hc_ctx::Graph& g, const hc::trans::Graph& out) {
    g.edges_out.swap(g.edges_next);
    g.o_out.swap(g.seq_next);
    g.out_off.swap(g.out_off_next);
    g.in_nodes.swap(g.in_nodes_next);
    g.in_off.swap(g.in_off_next);
    g.n_edges = out.E;
    g.n_tied = 0;  // the lists are in the reference's order now
    g.edits++;
}

int hc_graph_remove_inclusions(hc_ctx* c, hc_clean_counts* counts) {
    if (!c || !counts) return fail(HC_ERR_ARG, "hc_graph_remove_inclusions: null argument");
    memset(counts, 0, sizeof *counts);
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_remove_inclusions: no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, "hc_graph_remove_inclusions: the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first");
    HC_HIP(hipSetDevice(c->device));
    hc::trans::Graph in, out;
    int rc = clean_prepare(c, in, out);
    if (rc) return rc;
    const uint64_t E1 = g.n_edges ? g.n_edges : 1;
    if ((rc = g.incl_vtx.ensure((g.n_vertices + 1) * 4)) || (rc = g.incl_off.ensure((g.n_vertices + 1) * 8)) ||
        (rc = g.incl_edges.ensure(2 * E1 * sizeof(hc_edge_rec))))
        return rc;
    g.have_groups = false;
    if (g.n_edges == 0) {  // nothing to remove; every marked vertex has an empty group
        std::vector<uint8_t> bits(g.n_vertices);
        std::vector<uint32_t> vtx;
        if (g.n_vertices) HC_HIP(hipMemcpy(bits.data(), g.incl.p, g.n_vertices, hipMemcpyDeviceToHost));
        for (uint64_t v = 0; v < g.n_vertices; v++)
            if (bits[v]) vtx.push_back((uint32_t)v);
        std::vector<uint64_t> off(vtx.size() + 1, 0);
        if (!vtx.empty()) HC_HIP(hipMemcpy(g.incl_vtx.p, vtx.data(), vtx.size() * 4, hipMemcpyHostToDevice));
        HC_HIP(hipMemcpy(g.incl_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
        g.n_groups = vtx.size();
        g.n_group_edges = 0;
        g.have_groups = true;
        counts->edges_before = counts->edges_after = 0;
        return HC_OK;
    }
    const hipError_t e = hc::trans::remove_inclusions(in, g.incl.as<uint8_t>(), out, g.incl_vtx.as<uint32_t>(), g.incl_off.as<unsigned long long>(),
                                                      g.incl_edges.as<hc_edge_rec>(), &g.n_groups, &g.n_group_edges, counts, g.clean_temp.p,
                                                      g.clean_temp.cap, c->stream);
    if (e != hipSuccess) {
        g.valid = false;
        return fail(HC_ERR_HIP, std::string("hc_graph_remove_inclusions: ") + hipGetErrorString(e));
    }
    clean_commit(g, out);
    g.have_groups = true;
    return HC_OK;
}

int hc_graph_remove_transitive(hc_ctx* c, uint32_t remove_trans, uint32_t branch_reduction, hc_clean_counts* counts) {
    if (!c || !counts) return fail(HC_ERR_ARG, "hc_graph_remove_transitive: null argument");
    memset(counts, 0, sizeof *counts);
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_remove_transitive: no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, "hc_graph_remove_transitive: the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first");
    counts->edges_before = counts->edges_after = g.n_edges;
    if (remove_trans == 0 || g.n_edges == 0) return HC_OK;  // :939-941; an empty graph stays as it is
    HC_HIP(hipSetDevice(c->device));
    hc::trans::Graph in, out;
    int rc = clean_prepare(c, in, out);
    if (rc) return rc;
    const hipError_t e = hc::trans::remove_transitive(in, out, remove_trans, branch_reduction, counts, g.clean_temp.p, g.clean_temp.cap, c->stream);
    if (e != hipSuccess) {
        g.valid = false;
        return fail(HC_ERR_HIP, std::string("hc_graph_remove_transitive: ") + hipGetErrorString(e));
    }
    clean_commit(g, out);
    return HC_OK;
}

int hc_graph_fetch_inclusion_edges(hc_ctx* c, uint32_t* group_vertex, uint64_t* group_off, hc_edge_rec* edges, uint64_t cap, uint64_t* n_groups,
                                   uint64_t* n_edges) {
    if (!c || !n_groups || !n_edges) return fail(HC_ERR_ARG, "hc_graph_fetch_inclusion_edges: null argument");
    hc_ctx::Graph& g = c->graph;
    if (!g.have_groups) return fail(HC_ERR_STATE, "hc_graph_fetch_inclusion_edges: hc_graph_remove_inclusions has not run on this graph");
    *n_groups = g.n_groups;
    *n_edges = g.n_group_edges;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (group_vertex && g.n_groups) HC_HIP(hipMemcpyAsync(group_vertex, g.incl_vtx.p, g.n_groups * 4, hipMemcpyDeviceToHost, s));
    if (group_off) HC_HIP(hipMemcpyAsync(group_off, g.incl_off.p, (g.n_groups + 1) * 8, hipMemcpyDeviceToHost, s));
    const uint64_t k = std::min(cap, g.n_group_edges);
    if (edges && k) HC_HIP(hipMemcpyAsync(edges, g.incl_edges.p, k * sizeof(hc_edge_rec), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    return HC_OK;
}

// room for `want` bytes in a grow-only buffer whose first `have` bytes stay
static int grow_keeping(hc_scratch& b, size_t have, size_t want, hipStream_t s) {
    if (want <= b.cap) return HC_OK;
    const size_t room = std::max(want, 2 * b.cap);
    return b.grow_keep(room + room / 8, have, s);  // (an eighth of headroom, as hc_scratch::ensure)
}

static const char* const kTiedRefusal =
    ": the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first";

// the second half of both calls: branching_edges grows by the removed records, the cleaned graph takes the current one's place
static int commit_removed(hc_ctx* c, const char* who, const hc::trans::Graph& in, hc::trans::Graph& out, bool target_ordered, uint64_t n_removed) {
    hc_ctx::Graph& g = c->graph;
    int rc = grow_keeping(g.branching, g.n_branching * sizeof(hc_edge_rec), (g.n_branching + n_removed + 1) * sizeof(hc_edge_rec), c->stream);
    if (rc) return rc;
    const hipError_t e = hc::trans::commit_removed(in, out, target_ordered, g.branching.as<hc_edge_rec>() + g.n_branching, n_removed, g.clean_temp.p,
                                                   g.clean_temp.cap, c->stream);
    if (e != hipSuccess) {
        g.valid = false;
        return fail(HC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    g.n_branching += n_removed;
    clean_commit(g, out);
    return HC_OK;
}

}  // extern "C"

int hc::graph_clean_prepare(hc_ctx* c, hc::trans::Graph& in, hc::trans::Graph& out) { return clean_prepare(c, in, out); }
void hc::graph_clean_commit(hc_ctx* c, const hc::trans::Graph& out) { clean_commit(c->graph, out); }

// hc_br_reduce's edit (hc_api_br.cpp): n_missing records of d_missing are appended to branching_edges, then the listed records leave the
// graph with their adj_in entries and follow them (src/BranchReduction.cpp:83-85, :217-225).  rec / in_pos on the device, checked by the
// caller: distinct, below the graph's edges.
int hc::graph_remove_records(hc_ctx* c, const char* who, const uint32_t* d_rec, const uint32_t* d_in_pos, uint64_t n, const hc_edge_rec* d_missing,
                             uint64_t n_missing) {
    hc_ctx::Graph& g = c->graph;
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
    int rc = grow_keeping(g.branching, g.n_branching * sizeof(hc_edge_rec), (g.n_branching + n_missing + n + 1) * sizeof(hc_edge_rec), c->stream);
    if (rc) return rc;
    hc::trans::Graph in, out;
    if (g.n_edges && (rc = clean_prepare(c, in, out))) return rc;
    if (n_missing)
        HC_HIP(hipMemcpyAsync(g.branching.as<hc_edge_rec>() + g.n_branching, d_missing, n_missing * sizeof(hc_edge_rec), hipMemcpyDeviceToDevice, c->stream));
    g.n_branching += n_missing;
    if (!g.n_edges) {
        HC_HIP(hipStreamSynchronize(c->stream));
        return n ? fail(HC_ERR_ARG, std::string(who) + ": records to remove from a graph without edges") : HC_OK;
    }
    const hipError_t e = hc::trans::remove_records(in, out, d_rec, d_in_pos, (uint32_t)n, g.branching.as<hc_edge_rec>() + g.n_branching, g.clean_temp.p,
                                                   g.clean_temp.cap, c->stream);
    if (e != hipSuccess) {
        g.valid = false;
        return fail(HC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    g.n_branching += n;
    clean_commit(g, out);
    return HC_OK;
}

extern "C" {

int hc_graph_remove_tips(hc_ctx* c, uint32_t max_tip_len, const hc_read_geom* reads, uint64_t n_reads, hc_tip_counts* counts) {
    if (!c || !counts || (n_reads && !reads)) return fail(HC_ERR_ARG, "hc_graph_remove_tips: null argument");
    memset(counts, 0, sizeof *counts);
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
    if (n_reads >= (1ull << 31)) return fail(HC_ERR_ARG, "hc_graph_remove_tips: more than 2^31-1 reads");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_remove_tips: no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, std::string("hc_graph_remove_tips") + kTiedRefusal);
    counts->edges_before = counts->edges_after = g.n_edges;
    HC_HIP(hipSetDevice(c->device));
    if (g.n_edges == 0) return HC_OK;  // no list of more than one entry: no tips
    hipStream_t s = c->stream;
    hc::trans::Graph in, out;
    int rc = clean_prepare(c, in, out);
    if (rc) return rc;
    // the tip flags of earlier calls stay; reads beyond them start at 0
    const uint64_t had = g.n_tip_reads, flags = std::max(had, n_reads);
    if ((rc = grow_keeping(g.tip_reads, had, flags + 1, s)) || (rc = g.read_geom.ensure((n_reads + 1) * sizeof(hc_read_geom)))) return rc;
    // a refused call (read index out of range) must leave the flags as they were: it sets none, and the zeroed tail is not counted yet
    if (flags > had) HC_HIP(hipMemsetAsync(g.tip_reads.as<uint8_t>() + had, 0, flags - had, s));
    if (n_reads) HC_HIP(hipMemcpyAsync(g.read_geom.p, reads, n_reads * sizeof(hc_read_geom), hipMemcpyHostToDevice, s));
    bool in_range = false;
    const hipError_t e = hc::trans::find_tips(in, max_tip_len, g.read_geom.as<hc_read_geom>(), n_reads, g.tip_reads.as<uint8_t>(), flags, counts, &in_range,
                                              g.clean_temp.p, g.clean_temp.cap, s);
    if (e != hipSuccess) {
        g.valid = false;
        return fail(HC_ERR_HIP, std::string("hc_graph_remove_tips: ") + hipGetErrorString(e));
    }
    if (!in_range) {
        memset(counts, 0, sizeof *counts);
        return fail(HC_ERR_ARG, "hc_graph_remove_tips: a record's read1 / read2 is not below n_reads");
    }
    g.n_tip_reads = flags;
    if ((rc = commit_removed(c, "hc_graph_remove_tips", in, out, false, counts->n_removed))) return rc;
    counts->edges_after = g.n_edges;
    return HC_OK;
}

int hc_graph_remove_branches(hc_ctx* c, hc_branch_counts* counts) {
    if (!c || !counts) return fail(HC_ERR_ARG, "hc_graph_remove_branches: null argument");
    memset(counts, 0, sizeof *counts);
    c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_remove_branches: no graph on the device");
    if (g.n_tied) return fail(HC_ERR_STATE, std::string("hc_graph_remove_branches") + kTiedRefusal);
    counts->edges_before = counts->edges_after = g.n_edges;
    if (g.n_edges == 0) {  // every vertex is its own component
        counts->n_components = g.n_vertices;
        return HC_OK;
    }
    HC_HIP(hipSetDevice(c->device));
    hc::trans::Graph in, out;
    int rc = clean_prepare(c, in, out);
    if (rc) return rc;
    const hipError_t e = hc::trans::find_branches(in, counts, g.clean_temp.p, g.clean_temp.cap, c->stream);
    if (e != hipSuccess) {
        g.valid = false;
        return fail(HC_ERR_HIP, std::string("hc_graph_remove_branches: ") + hipGetErrorString(e));
    }
    if ((rc = commit_removed(c, "hc_graph_remove_branches", in, out, true, counts->n_removed))) return rc;
    counts->edges_after = g.n_edges;
    return HC_OK;
}

int hc_graph_fetch_branching_edges(hc_ctx* c, hc_edge_rec* edges, uint64_t cap, uint64_t* n_edges) {
    if (!c || !n_edges) return fail(HC_ERR_ARG, "hc_graph_fetch_branching_edges: null argument");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_fetch_branching_edges: no graph on the device");
    *n_edges = g.n_branching;
    const uint64_t k = std::min(cap, g.n_branching);
    if (edges && k) {
        HC_HIP(hipSetDevice(c->device));
        HC_HIP(hipMemcpyAsync(edges, g.branching.p, k * sizeof(hc_edge_rec), hipMemcpyDeviceToHost, c->stream));
        HC_HIP(hipStreamSynchronize(c->stream));
    }
    return HC_OK;
}

int hc_graph_fetch_tip_reads(hc_ctx* c, uint8_t* is_tip, uint64_t n_reads) {
    if (!c || (n_reads && !is_tip)) return fail(HC_ERR_ARG, "hc_graph_fetch_tip_reads: null argument");
    hc_ctx::Graph& g = c->graph;
    if (!g.valid) return fail(HC_ERR_STATE, "hc_graph_fetch_tip_reads: no graph on the device");
    const uint64_t k = std::min(n_reads, g.n_tip_reads);
    if (n_reads > k) memset(is_tip + k, 0, n_reads - k);
    if (k) {
        HC_HIP(hipSetDevice(c->device));
        HC_HIP(hipMemcpyAsync(is_tip, g.tip_reads.p, k, hipMemcpyDeviceToHost, c->stream));
        HC_HIP(hipStreamSynchronize(c->stream));
    }
    return HC_OK;
}

}  // extern "C"
