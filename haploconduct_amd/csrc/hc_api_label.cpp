// hc_api_label.cpp — hc_graph_label_vertices and hc_graph_fetch_orientations (include/hcedge.h): OverlapGraph::vertexLabellingHeuristic
// and checkDuplicateEdges on the graph the context holds.  The kernels are hc_label_kernels.hip's; the host decides between the phases
// (the refusal, whether any component holds an odd cycle, the best try) and walks the inconsistent components (host/Labelling.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcedge.h"
#include "hc_ctx.h"
#include "hc_label.h"
#include "host/Labelling.h"
#include "host/Types.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {
namespace lb = hc::label;

// the arrays of lb::Work in one block
size_t carve(lb::Work& w, char* base, uint64_t V, uint64_t E) {
    size_t at = 0;
    auto take = [&](auto*& p, uint64_t n) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = base ? (T*)(base + at) : nullptr;
        at += (n * sizeof(T) + 255) / 256 * 256;
    };
    const uint64_t E1 = E + 1, V1 = V + 1;
    take(w.src, E1), take(w.tgt, E1), take(w.same, E1);
    take(w.parent, 2 * V1), take(w.start, 2 * V1), take(w.L, 2 * V1);
    take(w.host_flag, V1), take(w.host_vtx, V1), take(w.lid, V1);
    take(w.sub_in_off, V1), take(w.sub_out_off, V1), take(w.sub_in, E1), take(w.sub_out, E1), take(w.sub_same, E1);
    take(w.bits, 2 * V1);
    take(w.rec_flag, E1), take(w.mv_sum, E1), take(w.keep_sum, E1), take(w.in_owner, E1), take(w.rm_in, V1);
    take(w.keys_a, E1), take(w.keys_b, E1), take(w.val_a, E1), take(w.val_b, E1);
    return at;
}
}  // namespace

extern "C" {

int hc_graph_label_vertices(hc_ctx* c, const hc_label_settings* st, hc_label_counts* counts) {
    const std::string me = "hc_graph_label_vertices: ";
    if (!c || !st || !counts) return fail(HC_ERR_ARG, me + "null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::Graph& g = c->graph;
    hc_ctx::Label& Q = c->label;
    if (!g.valid) return fail(HC_ERR_STATE, me + "no graph on the device");
    if (g.n_tied)
        return fail(HC_ERR_STATE, me + "the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first");
    const uint64_t V = g.n_vertices, E = g.n_edges;
    counts->edges_before = counts->edges_after = E;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    lb::Work w{};
    int rc;
    if ((rc = Q.work.ensure(carve(w, nullptr, V, E))) || (rc = Q.temp.ensure(lb::temp_bytes(E, V))) || (rc = Q.counters.ensure(lb::kCounters * 8)) ||
        (rc = Q.orient.ensure(V + 1)))
        return rc;
    carve(w, Q.work.as<char>(), V, E);
    w.orient = Q.orient.as<uint8_t>();
    w.counters = Q.counters.as<unsigned long long>();
    w.temp = Q.temp.p, w.temp_bytes = Q.temp.cap;
    hc::trans::Graph in, out;
    if ((rc = hc::graph_clean_prepare(c, in, out))) return rc;
    unsigned long long h[lb::kCounters];
    auto read_counters = [&]() -> hipError_t {
        const hipError_t e = hipMemcpyAsync(h, w.counters, sizeof h, hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };
    const bool resolve = (st->flags & HC_FLAG_RESOLVE_ORIENTATIONS) && !(st->flags & HC_FLAG_ADD_DUPLICATES);
    if (!resolve) {  // :185-192: no edge is touched
        std::vector<uint8_t> o(V, 1);
        if (st->flags & HC_FLAG_ADD_DUPLICATES)
            for (uint64_t v = st->n_reads; v < V; v++) o[v] = 0;
        if (V) HC_HIP(hipMemcpyAsync(w.orient, o.data(), V, hipMemcpyHostToDevice, s));
        HC_HIP(hipStreamSynchronize(s));
    } else {
        HC_HIP(lb::prepare(in, w, s));
        HC_HIP(read_counters());
        if (h[lb::kRepeated] != lb::kNoPlace) {  // the graph and the kept orientations stay as they are
            counts->status = HC_LABEL_REPEATED_RECORD;
            counts->bad_v = (uint32_t)(h[lb::kRepeated] >> 32), counts->bad_pos = (uint32_t)h[lb::kRepeated];
            return HC_OK;
        }
        Q.drop();
        c->graph_text.drop(), c->fno1.drop(), c->cliques.drop();
        HC_HIP(lb::components(in, w, s));
        HC_HIP(read_counters());
        counts->n_components = h[lb::kComponents];
        counts->n_inconsistent = h[lb::kInconsistent];
        const uint32_t n_host = (uint32_t)h[lb::kHostVertices], n_tries = n_host ? lb::kTries : 1;
        uint32_t best = 0;
        if (n_host) {  // the tries of the components with an odd cycle, on the host over their lists
            HC_HIP(lb::compact_subgraph(in, w, n_host, s));
            std::vector<uint64_t> in_off(n_host + 1), out_off(n_host + 1);
            HC_HIP(hipMemcpyAsync(in_off.data(), w.sub_in_off, (n_host + 1) * 8, hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(out_off.data(), w.sub_out_off, (n_host + 1) * 8, hipMemcpyDeviceToHost, s));
            HC_HIP(hipStreamSynchronize(s));
            const uint64_t n_in = in_off[n_host], n_out = out_off[n_host];
            std::vector<uint32_t> in_nb(n_in), out_nb(n_out);
            std::vector<uint8_t> out_same(n_out);
            if (n_in) HC_HIP(hipMemcpyAsync(in_nb.data(), w.sub_in, n_in * 4, hipMemcpyDeviceToHost, s));
            if (n_out) HC_HIP(hipMemcpyAsync(out_nb.data(), w.sub_out, n_out * 4, hipMemcpyDeviceToHost, s));
            if (n_out) HC_HIP(hipMemcpyAsync(out_same.data(), w.sub_same, n_out, hipMemcpyDeviceToHost, s));
            HC_HIP(hipStreamSynchronize(s));
            counts->n_host_vertices = n_host;
            counts->n_host_edges = n_out;
            std::vector<uint64_t> bits(2 * (size_t)n_host);
            try {
                const lb::Subgraph S{n_host, in_off.data(), out_off.data(), in_nb.data(), out_nb.data(), out_same.data()};
                lb::label_tries(S, n_tries, c->settings.n_threads ? c->settings.n_threads : 1, bits.data());
            } catch (const hc::FatalError& e) {
                return fail(e.status, me + e.what);
            }
            HC_HIP(hipMemcpyAsync(w.bits, bits.data(), bits.size() * 8, hipMemcpyHostToDevice, s));
            HC_HIP(lb::scatter_bits(w, n_host, s));
            HC_HIP(lb::conflicts(in, w, n_tries, s));
            HC_HIP(read_counters());  // (also: the copy has read `bits`)
            for (uint32_t t = 1; t < n_tries; t++)  // the first try with the strictly smallest count, :207
                if (h[lb::kTry0 + t] < h[lb::kTry0 + best]) best = t;
        }
        // from here on the records change in place: a failure leaves no graph
        hipError_t e = lb::apply(in, out, w, n_tries, best, s);
        if (e == hipSuccess) e = read_counters();
        if (e != hipSuccess) {
            g.valid = false;
            return fail(HC_ERR_HIP, me + hipGetErrorString(e));
        }
        counts->tries = n_tries;
        counts->best_try = best + 1;
        counts->n_moved = h[lb::kMoved];
        counts->n_switched = h[lb::kSwitched];
        counts->conflict_count = h[lb::kDeleted];
        if (E) {
            out.E = (uint32_t)(E - h[lb::kDeleted]);
            hc::graph_clean_commit(c, out);
            in = out;
        }
        counts->edges_after = g.n_edges;
    }
    Q.n_orient = V;
    Q.valid = true;
    // checkDuplicateEdges, src/OverlapGraph.cpp:578-605
    HC_HIP(lb::check_duplicates(in, w, s));
    HC_HIP(read_counters());
    if (h[lb::kDuplicate] != lb::kNoPlace) {
        counts->status = HC_LABEL_DUPLICATE_EDGE;
        counts->bad_v = (uint32_t)(h[lb::kDuplicate] >> 32), counts->bad_pos = (uint32_t)h[lb::kDuplicate];
    }
    return HC_OK;
}

int hc_graph_fetch_orientations(hc_ctx* c, uint8_t* vertex_fwd, uint64_t n_vertices) {
    if (!c || (n_vertices && !vertex_fwd)) return fail(HC_ERR_ARG, "hc_graph_fetch_orientations: null argument");
    const hc_ctx::Label& Q = c->label;
    if (!c->graph.valid || !Q.valid) return fail(HC_ERR_STATE, "hc_graph_fetch_orientations: no orientations on the device (hc_graph_label_vertices first)");
    if (n_vertices != Q.n_orient) return fail(HC_ERR_ARG, "hc_graph_fetch_orientations: one byte per vertex of the graph");
    if (!n_vertices) return HC_OK;
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(vertex_fwd, Q.orient.p, n_vertices, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

}  // extern "C"
