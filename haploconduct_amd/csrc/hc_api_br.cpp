// hc_api_br.cpp — hc_br_set_original_reads / hc_br_evidence / hc_br_evidence_fetch and hc_br_reduce / hc_br_reduce_fetch (include/hcsr.h).
// The first three: the read evidence of every branch of the
// device graph (BranchReduction::findBranchingEvidence, reference src/BranchReduction.cpp:229-743) from what the context holds — the graph,
// the kept store, the kept dict, the original reads — by the kernels of hc_br_kernels.hip around hc_prims' sums, sorts and selections.
// The host sizes the blocks between the phases (branches, neighbours and pairs; diff slots in use; items) and reads two flags; everything
// else stays on the device until hc_br_evidence_fetch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_br.h"
#include "hc_ctx.h"
#include "host/BranchReduce.h"
#include "hc_prims.h"
#include "hc_trans.h"

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

int bits_for(uint64_t n) {  // bits that hold every value below n
    int b = 1;
    while (b < 32 && (1ull << b) < n) b++;
    return b;
}

// arrays of one block, each on a 256-byte boundary; a first pass with base == nullptr sizes the block
struct Carve {
    char* base;
    size_t used = 0;
    template <typename T>
    T* take(uint64_t n) {
        const size_t at = (used + 255) & ~(size_t)255;
        used = at + (size_t)(n ? n : 1) * sizeof(T);
        return base ? (T*)(base + at) : nullptr;
    }
};

using hc::br::Work;

#define HC_BR_TAKE(field, n) W.field = c.take<std::remove_pointer_t<decltype(W.field)>>(n)
void carve_v(Carve& c, Work& W, uint64_t V, uint64_t E) {
    HC_BR_TAKE(cnt_b, 2 * V + 1), HC_BR_TAKE(cnt_s, 2 * V + 1), HC_BR_TAKE(cnt_p, 2 * V + 1), HC_BR_TAKE(in_key_a, E), HC_BR_TAKE(in_key_b, E);
    HC_BR_TAKE(rec_in, E), HC_BR_TAKE(rec_out, E), HC_BR_TAKE(rec_flag, E), HC_BR_TAKE(rec_sel, E);
}
void carve_b(Carve& c, Work& W, uint64_t nb, uint64_t ns, uint64_t np) {
    HC_BR_TAKE(br_node, nb), HC_BR_TAKE(nb_off, nb + 1), HC_BR_TAKE(pair_off, nb + 1), HC_BR_TAKE(diff_off, nb + 1), HC_BR_TAKE(br_status, nb);
    HC_BR_TAKE(br_node1len, nb), HC_BR_TAKE(br_dist, nb), HC_BR_TAKE(br_false, nb), HC_BR_TAKE(br_status8, nb);
    HC_BR_TAKE(sl_node, ns), HC_BR_TAKE(sl_rec, ns), HC_BR_TAKE(sl_len, ns), HC_BR_TAKE(sl_olen, ns), HC_BR_TAKE(nb_sel, ns), HC_BR_TAKE(sl_pos, ns);
    HC_BR_TAKE(sl_start, ns), HC_BR_TAKE(sl_seq, ns), HC_BR_TAKE(sl_items, ns + 1), HC_BR_TAKE(sl_item_off, ns + 1), HC_BR_TAKE(sl_paired, ns);
    HC_BR_TAKE(sl_keep, ns), HC_BR_TAKE(pr_raw, np), HC_BR_TAKE(pr_cnt, np + 1), HC_BR_TAKE(pr_off, np + 1), HC_BR_TAKE(pr_info, np), HC_BR_TAKE(miss_sel, np);
    HC_BR_TAKE(pr_term, np), HC_BR_TAKE(pr_rel, np), HC_BR_TAKE(pr_len, np), HC_BR_TAKE(pr_diff, np * HC_BR_MAX_DIFFS), HC_BR_TAKE(pr_miss, np);
}
void carve_d(Carve& c, Work& W, uint64_t nd) { HC_BR_TAKE(dk_in, nd), HC_BR_TAKE(dk, nd), HC_BR_TAKE(d_flag, nd), HC_BR_TAKE(d_sel, nd), HC_BR_TAKE(d_branch, nd); }
void carve_e(Carve& c, Work& W, uint64_t nk) { HC_BR_TAKE(ek_in, nk), HC_BR_TAKE(ek, nk), HC_BR_TAKE(e_flag, nk), HC_BR_TAKE(e_sel, nk), HC_BR_TAKE(e_rec, nk); }
#undef HC_BR_TAKE

template <typename F>
int room(hc_scratch& block, F carve) {  // size, allocate, carve
    Carve sizing{nullptr};
    carve(sizing);
    const int rc = block.ensure(sizing.used + 256);
    if (rc) return rc;
    Carve c{(char*)(((uintptr_t)block.p + 255) & ~(uintptr_t)255)};
    carve(c);
    return HC_OK;
}

}  // namespace

extern "C" {

int hc_br_set_original_reads(hc_ctx* c, const uint8_t* bases, const uint64_t* seq_off, uint64_t n_reads) {
    const char* me = "hc_br_set_original_reads";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    if (const char* what = hc::br::check_original_reads(bases, seq_off, n_reads)) return fail(me, HC_ERR_ARG, what);
    hc_ctx::Br& B = c->br;
    HC_HIP(hipSetDevice(c->device));
    const uint64_t total = seq_off[n_reads];
    hc_scratch nb, no;  // any error leaves the kept reads as they were
    int rc;
    if ((rc = nb.ensure(total ? total : 1)) || (rc = no.ensure((n_reads + 1) * 8))) return rc;
    if (total) HC_HIP(hipMemcpyAsync(nb.p, bases, total, hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipMemcpyAsync(no.p, seq_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    B.orig_bases.swap(nb);
    B.orig_off.swap(no);
    B.n_orig = n_reads;
    B.orig_valid = true;
    return HC_OK;
}

int hc_br_evidence(hc_ctx* c, const uint32_t* vertex_read, const uint8_t* vertex_fwd, uint64_t n_vertices, const hc_br_settings* st, hc_br_counts* counts) {
    const char* me = "hc_br_evidence";
    if (!c || !st || !counts) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::Br& B = c->br;
    hc_ctx::Graph& g = c->graph;
    B.drop();
    if (!g.valid) return fail(me, HC_ERR_STATE, "no graph on the device");
    if (g.n_tied)
        return fail(me, HC_ERR_STATE, "the device holds out-lists whose order only the host knows (hc_graph_resolve's tied lists): hc_graph_load the host's lists first");
    if (!c->have_reads || !c->srn.keep || !c->srn.raw_valid) return fail(me, HC_ERR_STATE, "no store loaded with hc_sr_keep_device on");
    if (!c->sr_orig.valid || c->sr_orig.n_reads != c->view.n_reads) return fail(me, HC_ERR_STATE, "no kept dict over the reads of the store");
    if (!B.orig_valid) return fail(me, HC_ERR_STATE, "no original reads (hc_br_set_original_reads first)");
    const uint64_t V = g.n_vertices, E = g.n_edges, n_reads = c->view.n_reads;
    if (n_vertices != V) return fail(me, HC_ERR_ARG, "n_vertices is not the graph's");
    if (E >= (1ull << 31) || V >= (1ull << 31)) return fail(me, HC_ERR_ARG, "2^31 edges or vertices or more");  // (the keys hold 31 bits of record)
    if (V && (!vertex_read || !vertex_fwd)) return fail(me, HC_ERR_ARG, "null vertex table");
    if (const char* what = hc::br::check_settings(st, B.n_orig)) return fail(me, HC_ERR_ARG, what);
    for (uint64_t v = 0; v < V; v++)
        if (vertex_read[v] >= n_reads) return fail(me, HC_ERR_ARG, "a vertex_read is no read of the store");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    float ms = 0;
    double ms_device = 0;
    // sortAdjOut's side effect (:48): the records in target order, by hc_graph_remove_branches' step (timed with the rest: its host step
    // for lists that repeat a target lies between the two events too)
    c->graph_text.drop(), c->fno1.drop();
    if (E) {
        HC_HIP(hipEventRecord(c->ev0, s));
        const uint64_t E1 = E;
        if ((rc = g.edges_next.ensure(E1 * sizeof(hc_edge_rec))) || (rc = g.seq_next.ensure(E1 * 4)) || (rc = g.clean_temp.ensure(hc::trans::temp_bytes(E, V))))
            return rc;
        const hc::trans::Graph in{g.edges_out.as<hc_edge_rec>(), g.o_out.as<uint32_t>(), g.out_off.as<unsigned long long>(), g.in_nodes.as<uint32_t>(),
                                  g.in_off.as<unsigned long long>(), (uint32_t)V, (uint32_t)E};
        hc::trans::Graph out{g.edges_next.as<hc_edge_rec>(), g.seq_next.as<uint32_t>(), nullptr, nullptr, nullptr, (uint32_t)V, (uint32_t)E};
        uint64_t n_tied = 0;
        const hipError_t e = hc::trans::sort_adj_out(in, out, &n_tied, g.clean_temp.p, g.clean_temp.cap, s);
        if (e != hipSuccess) {
            g.valid = false;
            return fail(me, HC_ERR_HIP, hipGetErrorString(e));
        }
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
        g.edges_out.swap(g.edges_next);
        g.o_out.swap(g.seq_next);
        g.sorted_at = ~0ull;  // the lists have left hc_graph_sort_edges' order (this swap does not pass through the cleaning calls' commit)
    }
    Work W{};
    hc::br::In I{};
    I.g = hc::br::Graph{g.edges_out.as<hc_edge_rec>(), g.out_off.as<uint64_t>(), g.in_nodes.as<uint32_t>(), g.in_off.as<uint64_t>(), (uint32_t)V, (uint32_t)E};
    I.st = hc::br::Store{c->srn.bases.as<uint8_t>(), c->srn.off.as<uint64_t>(), c->srn.first.as<uint32_t>(), (uint32_t)n_reads};
    I.d = hc::br::Dict{c->sr_orig.off.as<uint64_t>(), c->sr_orig.entries.as<hc_sr_original>()};
    I.o = hc::br::Originals{B.orig_bases.as<uint8_t>(), B.orig_off.as<uint64_t>(), B.n_orig};
    I.se = st->se_count, I.pe = st->pe_count, I.orc = st->original_readcount;
    I.min_overlap_len = st->min_overlap_len;
    I.edge_threshold = st->edge_threshold;
    const uint64_t nv2 = 2 * V + 1;
    if ((rc = B.vread.ensure((V + 1) * 4)) || (rc = B.vfwd.ensure(V + 1)) || (rc = B.counters.ensure(hc::br::kCounters * 8)) ||
        (rc = room(B.work_v, [&](Carve& k) { carve_v(k, W, V, E); })) ||
        (rc = B.temp.ensure(std::max({hc::prims::scan_temp_bytes(nv2, 8), hc::prims::sort_temp_bytes(E ? E : 1, 8, 4), hc::prims::select_temp_bytes(E + 1)}))))
        return rc;
    W.counters = B.counters.as<unsigned long long>();
    I.vread = B.vread.as<uint32_t>();
    I.vfwd = B.vfwd.as<uint8_t>();
    if (V) {
        HC_HIP(hipMemcpyAsync(B.vread.p, vertex_read, V * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(B.vfwd.p, vertex_fwd, V, hipMemcpyHostToDevice, s));
    }
    HC_HIP(hipStreamSynchronize(s));  // (the copies are not the device's time)
    auto timed = [&]() -> int {
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
        return HC_OK;
    };
    // A: the branches, their neighbours and pairs
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hipMemsetAsync(W.counters, 0, hc::br::kCounters * 8, s));
    HC_HIP(hc::br::launch_count(I, W, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.cnt_b, W.cnt_b, nv2, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.cnt_s, W.cnt_s, nv2, s));
    HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.cnt_p, W.cnt_p, nv2, s));
    if (E) {
        HC_HIP(hc::br::launch_in_keys(I, W, s));
        HC_HIP(hc::prims::sort_keys(B.temp.p, B.temp.cap, W.in_key_a, W.in_key_b, E, 0, 32 + bits_for(V), s));
    }
    uint64_t h[4] = {0, 0, 0, 0};
    HC_HIP(hipMemcpyAsync(&h[0], W.cnt_b + 2 * V, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&h[1], W.cnt_b + V, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&h[2], W.cnt_s + 2 * V, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&h[3], W.cnt_p + 2 * V, 8, hipMemcpyDeviceToHost, s));
    if ((rc = timed())) return rc;
    const uint64_t nb = h[0], ns = h[2], np = h[3];
    W.n_b = nb, W.n_in = h[1], W.n_s = ns, W.n_p = np;
    if (np * HC_BR_MAX_DIFFS >= (1ull << 32)) return fail(me, HC_ERR_ARG, "2^32 / 100 neighbour pairs or more");
    hc_br_counts cn;
    memset(&cn, 0, sizeof cn);
    cn.n_branches = nb;
    uint64_t n_items = 0;
    std::vector<uint8_t> status(nb);
    if (nb) {
        const uint64_t most = std::max({ns, np, nb}) + 1;
        if ((rc = room(B.work_b, [&](Carve& k) { carve_b(k, W, nb, ns, np); })) ||
            (rc = B.temp.ensure(std::max({hc::prims::scan_temp_bytes(most, 8), hc::prims::select_temp_bytes(most), B.temp.cap}))) ||
            (rc = B.t_branches.ensure(nb * sizeof(hc_br_branch))) || (rc = B.t_nb.ensure(ns * 4)))
            return rc;
        W.t_branches = B.t_branches.as<hc_br_branch>();
        W.t_nb = B.t_nb.as<uint32_t>();
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::br::launch_branches(I, W, s));
        HC_HIP(hc::br::launch_slots(I, W, s));
        HC_HIP(hc::br::launch_branch_geometry(I, W, s));
        HC_HIP(hc::br::launch_pairs(I, W, s));
        unsigned long long flags[hc::br::kCounters];
        HC_HIP(hipMemcpyAsync(flags, W.counters, sizeof flags, hipMemcpyDeviceToHost, s));
        if ((rc = timed())) return rc;
        if (flags[hc::br::kCntArgError])
            return fail(me, HC_ERR_ARG, "a neighbour's record is missing from adj_out or names a read that is no read of the store");
        // B - D; once more where an item found a bad original (the branch's lists are laid out by then)
        for (int pass = 0; pass < 2; pass++) {
            HC_HIP(hipEventRecord(c->ev0, s));
            HC_HIP(hipMemsetAsync(W.counters, 0, hc::br::kCounters * 8, s));
            HC_HIP(hc::br::launch_branch_verdict(I, W, s));
            HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.pr_cnt, W.pr_off, np + 1, s));
            HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, W.sl_items, W.sl_item_off, ns + 1, s));
            HC_HIP(hc::prims::select_flagged(B.temp.p, B.temp.cap, W.sl_keep, ns, W.nb_sel, W.counters + hc::br::kCntNbSel, s));
            HC_HIP(hc::prims::select_flagged(B.temp.p, B.temp.cap, W.pr_miss, np, W.miss_sel, W.counters + hc::br::kCntMissSel, s));
            HC_HIP(hc::br::launch_nb_gather(W, s));
            uint32_t nd32 = 0;
            HC_HIP(hipMemcpyAsync(&nd32, W.pr_off + np, 4, hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(&n_items, W.sl_item_off + ns, 8, hipMemcpyDeviceToHost, s));
            if ((rc = timed())) return rc;
            const uint64_t nd = nd32, nk = 2 * n_items;
            if (n_items >= (1ull << 31)) return fail(me, HC_ERR_ARG, "2^31 items or more");
            if ((rc = room(B.work_d, [&](Carve& k) { carve_d(k, W, nd); })) || (rc = room(B.work_e, [&](Carve& k) { carve_e(k, W, nk); })) ||
                (rc = B.temp.ensure(std::max({hc::prims::sort_temp_bytes(std::max<uint64_t>({nd, nk, 1}), 8, 4),
                                              hc::prims::select_temp_bytes(std::max<uint64_t>({nd, nk, 1})), B.temp.cap}))) ||
                (rc = B.t_diff.ensure((nd ? nd : 1) * 4)) || (rc = B.t_ev_ids.ensure((nk ? nk : 1) * 4)) || (rc = B.t_ev_edge.ensure((E ? E : 1) * 8)) ||
                (rc = B.t_ev_off.ensure((E + 1) * 8)) || (rc = B.t_missing.ensure((np ? np : 1) * sizeof(hc_edge_rec))))
                return rc;
            W.t_diff = B.t_diff.as<int32_t>();
            W.t_ev_ids = B.t_ev_ids.as<uint32_t>();
            W.t_ev_edge = B.t_ev_edge.as<uint32_t>();
            W.t_ev_off = B.t_ev_off.as<uint64_t>();
            W.t_missing = B.t_missing.as<hc_edge_rec>();
            HC_HIP(hipEventRecord(c->ev0, s));
            if (nd) {
                HC_HIP(hc::br::launch_diff_keys(W, nd, s));
                HC_HIP(hc::prims::sort_keys(B.temp.p, B.temp.cap, W.dk_in, W.dk, nd, 0, 32 + bits_for(nb), s));
                HC_HIP(hc::br::launch_diff_first(W, nd, s));
                HC_HIP(hc::prims::select_flagged(B.temp.p, B.temp.cap, W.d_flag, nd, W.d_sel, W.counters + hc::br::kCntDiffSel, s));
                HC_HIP(hc::br::launch_diff_gather(W, nd, s));
            }
            HC_HIP(hc::br::launch_diff_offsets(W, s));
            // C, D
            if (E) {
                HC_HIP(hipMemsetAsync(W.rec_in, 0, E, s));
                HC_HIP(hipMemsetAsync(W.rec_out, 0, E, s));
                HC_HIP(hipMemsetAsync(W.rec_flag, 0, E, s));
            }
            HC_HIP(hc::br::launch_record_flags(W, s));
            if (nk) {
                HC_HIP(hc::br::launch_items(I, W, n_items, s));
                HC_HIP(hc::prims::sort_keys(B.temp.p, B.temp.cap, W.ek_in, W.ek, nk, 0, 33 + bits_for(E + 1), s));
                HC_HIP(hc::br::launch_ev_keep(I, W, nk, s));
                HC_HIP(hc::prims::select_flagged(B.temp.p, B.temp.cap, W.e_flag, nk, W.e_sel, W.counters + hc::br::kCntEvSel, s));
                HC_HIP(hc::br::launch_ev_gather(W, nk, s));
            }
            if (E) HC_HIP(hc::prims::select_flagged(B.temp.p, B.temp.cap, W.rec_flag, E, W.rec_sel, W.counters + hc::br::kCntRecSel, s));
            HC_HIP(hc::br::launch_ev_edges(I, W, s));
            HC_HIP(hc::br::launch_missing(I, W, s));
            HC_HIP(hc::br::launch_assemble(W, s));
            HC_HIP(hipMemcpyAsync(flags, W.counters, sizeof flags, hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(status.data(), W.br_status8, nb, hipMemcpyDeviceToHost, s));
            if ((rc = timed())) return rc;
            cn.n_branch_nb = flags[hc::br::kCntNbSel];
            cn.n_diff = flags[hc::br::kCntDiffSel];
            cn.n_ev_edges = flags[hc::br::kCntRecSel];
            cn.n_ev_ids = flags[hc::br::kCntEvSel];
            cn.n_missing = flags[hc::br::kCntMissSel];
            if (!flags[hc::br::kCntBadOriginal]) break;
            if (pass == 1) return fail(me, HC_ERR_STATE, "a branch failed in the second pass only");
        }
    }
    cn.n_items = n_items;
    for (uint8_t x : status) cn.n_failed += x != HC_BR_OK;
    cn.ms_device = ms_device;
    B.counts = cn;
    B.valid = true;
    B.sl_rec = W.sl_rec, B.nb_sel = W.nb_sel;  // (work_b stays as it is until the next call)
    B.graph_edits = g.edits;
    B.settings_orc = st->original_readcount;
    *counts = cn;
    return cn.n_failed ? HC_BR_SOME_FAILED : HC_OK;
}

int hc_br_evidence_fetch(hc_ctx* c, hc_br_tables* T) {
    const char* me = "hc_br_evidence_fetch";
    if (!c || !T) return fail(me, HC_ERR_ARG, "null argument");
    const hc_ctx::Br& B = c->br;
    if (!B.valid) return fail(me, HC_ERR_STATE, "no tables on the device (hc_br_evidence first)");
    const hc_br_counts& n = B.counts;
    if ((T->branches && T->cap_branches < n.n_branches) || (T->branch_nb && T->cap_branch_nb < n.n_branch_nb) || (T->diff_pos && T->cap_diff < n.n_diff) ||
        ((T->ev_edge || T->ev_off) && T->cap_ev_edges < n.n_ev_edges) || (T->ev_ids && T->cap_ev_ids < n.n_ev_ids) ||
        (T->missing_edges && T->cap_missing < n.n_missing))
        return fail(me, HC_ERR_ARG, "a table is too small (hc_br_evidence returned the counts)");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    auto down = [&](void* dst, const hc_scratch& k, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, k.p, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
    HC_HIP(down(T->branches, B.t_branches, n.n_branches * sizeof(hc_br_branch)));
    HC_HIP(down(T->branch_nb, B.t_nb, n.n_branch_nb * 4));
    HC_HIP(down(T->diff_pos, B.t_diff, n.n_diff * 4));
    HC_HIP(down(T->ev_edge, B.t_ev_edge, n.n_ev_edges * 8));
    if (T->ev_off) {
        if (n.n_branches) HC_HIP(down(T->ev_off, B.t_ev_off, (n.n_ev_edges + 1) * 8));
        else T->ev_off[0] = 0;
    }
    HC_HIP(down(T->ev_ids, B.t_ev_ids, n.n_ev_ids * 4));
    HC_HIP(down(T->missing_edges, B.t_missing, n.n_missing * sizeof(hc_edge_rec)));
    HC_HIP(hipStreamSynchronize(s));
    return HC_OK;
}

}  // extern "C"

// ---- hc_br_reduce ----------------------------------------------------------------------------------------------------------------------
// Five phases around two host steps (host/BranchReduce.h, shared with the mirror): the records' lengths for the walk; THE WALK; the unique
// evidence of every component edge and the general rule; THE CHAIN; the records of edges_to_remove and the edit.  What crosses the link is
// per branch and per component edge, never per evidence id — unless a component has to be finished from the lists themselves (an edge
// without a row, an edge in two components: neither can come from hc_br_evidence's tables), when the evidence tables are fetched whole.

namespace {

using hc::br::Red;
using hc::brr::node_pair_t;

void carve_red_edges(Carve& c, Red& R, uint64_t n_ce, uint64_t n_c, uint64_t n_rm) {
    R.ce_u = c.take<uint32_t>(n_ce), R.ce_v = c.take<uint32_t>(n_ce), R.ce_comp = c.take<uint32_t>(n_ce), R.ce_row = c.take<uint32_t>(n_ce);
    R.ce_count = c.take<uint32_t>(n_ce), R.ce_len = c.take<uint64_t>(n_ce + 1), R.ce_off = c.take<uint64_t>(n_ce + 1), R.ce_remove = c.take<uint8_t>(n_ce);
    R.cm_first = c.take<uint64_t>(n_c + 1), R.cm_minev = c.take<int32_t>(n_c), R.cm_no_row = c.take<uint8_t>(n_c), R.cm_keep = c.take<uint8_t>(n_c);
    R.rm_u = c.take<uint32_t>(n_rm), R.rm_v = c.take<uint32_t>(n_rm), R.rm_rec = c.take<uint32_t>(n_rm), R.rm_in = c.take<uint32_t>(n_rm);
}
void carve_red_items(Carve& c, Red& R, uint64_t n) {
    R.key_in = c.take<uint64_t>(n), R.key = c.take<uint64_t>(n), R.uniq = c.take<uint64_t>(n + 1), R.val_in = c.take<uint32_t>(n), R.val = c.take<uint32_t>(n);
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

extern "C" {

int hc_br_reduce(hc_ctx* c, const hc_br_reduce_settings* st, hc_br_reduce_counts* counts) {
    const char* me = "hc_br_reduce";
    if (!c || !st || !counts) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::Br& B = c->br;
    hc_ctx::Graph& g = c->graph;
    if (!B.valid) return fail(me, HC_ERR_STATE, "no tables on the device (hc_br_evidence first; a reduction spends them)");
    if (!g.valid || g.n_tied || g.edits != B.graph_edits) return fail(me, HC_ERR_STATE, "the graph was replaced or cleaned since hc_br_evidence");
    if (!c->have_reads || !c->srn.keep || !c->srn.raw_valid) return fail(me, HC_ERR_STATE, "the store hc_br_evidence read is no longer kept");
    if (!st->n_thresholds || !st->thresholds) return fail(me, HC_ERR_ARG, "an empty threshold table (the exit(1) of src/BranchReduction.cpp:157)");
    B.valid = false;  // spent, whatever happens from here on
    B.red_valid = false;
    const uint64_t V = g.n_vertices, E = g.n_edges;
    const uint64_t n_b = B.counts.n_branches, n_nb = B.counts.n_branch_nb, n_rows = B.counts.n_ev_edges, n_ids = B.counts.n_ev_ids, n_missing = B.counts.n_missing;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    float ms = 0;
    double ms_device = 0, ms_copy = 0, ms_walk = 0, ms_sort = 0, ms_edit = 0;
    auto timed = [&]() -> int {
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
        return HC_OK;
    };
    const hc::br::Graph dg{g.edges_out.as<hc_edge_rec>(), g.out_off.as<uint64_t>(), g.in_nodes.as<uint32_t>(), g.in_off.as<uint64_t>(), (uint32_t)V, (uint32_t)E};
    const hc::br::Store ds{c->srn.bases.as<uint8_t>(), c->srn.off.as<uint64_t>(), c->srn.first.as<uint32_t>(), (uint32_t)c->view.n_reads};
    Red R{};
    R.nb_sel = B.nb_sel, R.sl_rec = B.sl_rec, R.n_nb = n_nb;
    R.ev_edge = B.t_ev_edge.as<uint32_t>(), R.ev_off = B.t_ev_off.as<uint64_t>(), R.ev_ids = B.t_ev_ids.as<uint32_t>(), R.n_rows = n_rows;
    R.id_limit = 2 * B.settings_orc;
    R.id_bits = bits_for(R.id_limit);
    if ((rc = B.counters.ensure(hc::br::kCounters * 8))) return rc;
    R.counters = B.counters.as<unsigned long long>();
    unsigned long long flags[hc::br::kRedCounters];
    // 1: what the walk asks getEdgeInfo for, with the branches and their neighbours, through the page-locked block
    std::vector<hc_br_branch> branches(n_b);
    std::vector<uint32_t> nb(n_nb);
    std::vector<hc::brr::Triple> tri(n_nb ? n_nb : 1);
    static_assert(sizeof(hc::brr::Triple) == 12, "three int32 per neighbour");
    if (n_b) {
        const size_t b_bytes = n_b * sizeof(hc_br_branch), nb_bytes = n_nb * 4, tri_bytes = n_nb * 12;
        const size_t nb_at = (b_bytes + 255) & ~(size_t)255, tri_at = (nb_at + nb_bytes + 255) & ~(size_t)255;
        if ((rc = room(B.red_work, [&](Carve& k) { R.tri = k.take<int32_t>(3 * n_nb); })) || (rc = B.red_pin.ensure(tri_at + tri_bytes + 256))) return rc;
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hipMemsetAsync(R.counters, 0, hc::br::kRedCounters * 8, s));
        if (n_nb) HC_HIP(hc::br::launch_red_triples(dg, ds, R, s));
        if ((rc = timed())) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        char* pin = (char*)B.red_pin.p;
        HC_HIP(hipMemcpyAsync(pin, B.t_branches.p, b_bytes, hipMemcpyDeviceToHost, s));
        if (n_nb) {
            HC_HIP(hipMemcpyAsync(pin + nb_at, B.t_nb.p, nb_bytes, hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(pin + tri_at, R.tri, tri_bytes, hipMemcpyDeviceToHost, s));
        }
        HC_HIP(hipMemcpyAsync(flags, R.counters, sizeof flags, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        memcpy(branches.data(), pin, b_bytes);
        if (n_nb) memcpy(nb.data(), pin + nb_at, nb_bytes), memcpy(tri.data(), pin + tri_at, tri_bytes);
        ms_copy += ms_since(t0);
        if (flags[hc::br::kRedBadRead]) return fail(me, HC_ERR_ARG, "a neighbour's record names a read that is no read of the store");
    }
    // 2: the walk
    hc::brr::Components cs;
    std::vector<int32_t> min_evidence;
    std::vector<uint8_t> found;
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (const char* what = hc::brr::find_components(branches.data(), n_b, nb.data(), n_nb, tri.data(), V, cs)) return fail(me, HC_ERR_ARG, what);
        hc::brr::mark_host_finished(cs, st->diploid != 0);
        hc::brr::look_up_thresholds(st, cs, min_evidence, found);
        ms_walk += ms_since(t0);
    }
    const uint64_t n_c = cs.comps.size(), n_ce = cs.edges.size();
    if (n_ce >= (1ull << 32) || n_ids >= (1ull << 32)) return fail(me, HC_ERR_ARG, "2^32 component edges or evidence ids or more");
    // 3: the unique evidence of every component edge, and the general rule
    std::vector<uint32_t> unique(n_ce ? n_ce : 1, 0);
    std::vector<uint8_t> ce_remove(n_ce ? n_ce : 1, 0), cm_keep(n_c ? n_c : 1, 0), cm_no_row(n_c ? n_c : 1, 0);
    R.n_ce = n_ce, R.n_c = n_c;
    if ((rc = room(B.red_work, [&](Carve& k) { carve_red_edges(k, R, n_ce, n_c, n_nb); }))) return rc;  // (edges_to_remove holds final_branch edges: <= n_nb)
    if (n_ce) {
        // up: u, v, component per edge; first edge and min_evidence per component
        const size_t e4 = (n_ce * 4 + 255) & ~(size_t)255, c8 = ((n_c + 1) * 8 + 255) & ~(size_t)255, c4 = (n_c * 4 + 255) & ~(size_t)255;
        if ((rc = B.red_pin.ensure(4 * e4 + c8 + c4 + n_ce + 2 * n_c + 1024))) return rc;
        char* pin = (char*)B.red_pin.p;
        uint32_t *hu = (uint32_t*)pin, *hv = (uint32_t*)(pin + e4), *hc_ = (uint32_t*)(pin + 2 * e4);
        uint64_t* hfirst = (uint64_t*)(pin + 3 * e4);
        int32_t* hmin = (int32_t*)(pin + 3 * e4 + c8);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t i = 0; i < n_c; i++) {
            hfirst[i] = cs.comps[i].edge_first;
            hmin[i] = min_evidence[i];
            for (uint64_t k = 0; k < cs.comps[i].edge_count; k++) {
                const uint64_t e = cs.comps[i].edge_first + k;
                hu[e] = (uint32_t)cs.edges[e].first, hv[e] = (uint32_t)cs.edges[e].second, hc_[e] = (uint32_t)i;
            }
        }
        hfirst[n_c] = n_ce;
        HC_HIP(hipMemcpyAsync(R.ce_u, hu, n_ce * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(R.ce_v, hv, n_ce * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(R.ce_comp, hc_, n_ce * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(R.cm_first, hfirst, (n_c + 1) * 8, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(R.cm_minev, hmin, n_c * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipStreamSynchronize(s));
        ms_copy += ms_since(t0);
        if ((rc = B.temp.ensure(std::max({hc::prims::scan_temp_bytes(n_ce + 1, 8), B.temp.cap})))) return rc;
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hipMemsetAsync(R.counters, 0, hc::br::kRedCounters * 8, s));
        HC_HIP(hipMemsetAsync(R.cm_no_row, 0, n_c, s));
        HC_HIP(hc::br::launch_red_rows(R, s));
        HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, R.ce_len, R.ce_off, n_ce + 1, s));
        uint64_t n_items = 0;
        HC_HIP(hipMemcpyAsync(&n_items, R.ce_off + n_ce, 8, hipMemcpyDeviceToHost, s));
        if ((rc = timed())) return rc;
        if (n_items > n_ids) return fail(me, HC_ERR_STATE, "more items than the tables hold ids");
        R.n_items = n_items;
        counts->n_items_sorted = n_items;
        if ((rc = room(B.work_e, [&](Carve& k) { carve_red_items(k, R, n_items); })) ||
            (rc = B.temp.ensure(std::max({hc::prims::sort_temp_bytes(n_items ? n_items : 1, 8, 4), hc::prims::scan_temp_bytes(n_items + 1, 8), B.temp.cap}))))
            return rc;
        HC_HIP(hipEventRecord(c->ev0, s));
        if (n_items) {
            HC_HIP(hc::br::launch_red_keys(R, s));
            if ((rc = timed())) return rc;
            HC_HIP(hipEventRecord(c->ev0, s));
            HC_HIP(hc::prims::sort_pairs(B.temp.p, B.temp.cap, R.key_in, R.key, R.val_in, R.val, n_items, 0, R.id_bits + bits_for(n_c), s));
            if ((rc = timed())) return rc;
            ms_sort += ms;
            HC_HIP(hipEventRecord(c->ev0, s));
        }
        HC_HIP(hc::br::launch_red_unique(R, s));
        HC_HIP(hc::prims::exclusive_sum(B.temp.p, B.temp.cap, R.uniq, R.uniq, n_items + 1, s));
        HC_HIP(hc::br::launch_red_counts(R, s));
        HC_HIP(hc::br::launch_red_decide(R, s));
        if ((rc = timed())) return rc;
        // down: the counts, the rule's bytes, the marks
        const auto t1 = std::chrono::steady_clock::now();
        uint8_t* hb = (uint8_t*)(pin + e4);
        HC_HIP(hipMemcpyAsync(pin, R.ce_count, n_ce * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(hb, R.ce_remove, n_ce, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(hb + n_ce, R.cm_keep, n_c, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(hb + n_ce + n_c, R.cm_no_row, n_c, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(flags, R.counters, sizeof flags, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        memcpy(unique.data(), pin, n_ce * 4);
        memcpy(ce_remove.data(), hb, n_ce), memcpy(cm_keep.data(), hb + n_ce, n_c), memcpy(cm_no_row.data(), hb + n_ce + n_c, n_c);
        ms_copy += ms_since(t1);
        if (flags[hc::br::kRedBadId]) return fail(me, HC_ERR_ARG, "an evidence id is not below 2 * original_readcount (the assert of :1068)");
    }
    // 4: the chain.  A component with an edge that has no row, or that shares an edge, is finished from the lists themselves.  (No tables of
    // hc_br_evidence mark a component so — include/hcsr.h says why —: this fetch runs in no test; count_unique and decide, which it hands
    // the lists to, are tested through the mirror.)  The marks but the no-row one are the host's (mark_host_finished in the walk).
    bool need_lists = false;
    for (uint64_t i = 0; i < n_c; i++) {
        if (cm_no_row[i]) cs.comps[i].host_finished |= HC_BR_RED_HOST_NO_ROW;
        need_lists |= (cs.comps[i].host_finished & (HC_BR_RED_HOST_NO_ROW | HC_BR_RED_HOST_SHARED_EDGE)) != 0;
    }
    std::vector<uint32_t> l_edge, l_ids;
    std::vector<uint64_t> l_off(1, 0);
    if (need_lists) {
        const auto t0 = std::chrono::steady_clock::now();
        l_edge.resize(2 * n_rows), l_off.resize(n_rows + 1), l_ids.resize(n_ids);
        if (n_rows) {
            HC_HIP(hipMemcpyAsync(l_edge.data(), B.t_ev_edge.p, n_rows * 8, hipMemcpyDeviceToHost, s));
            HC_HIP(hipMemcpyAsync(l_off.data(), B.t_ev_off.p, (n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
        }
        if (n_ids) HC_HIP(hipMemcpyAsync(l_ids.data(), B.t_ev_ids.p, n_ids * 4, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        ms_copy += ms_since(t0);
    }
    {
        const auto t0 = std::chrono::steady_clock::now();
        hc::brr::Evidence lists(l_edge.data(), l_off.data(), l_ids.data(), need_lists ? n_rows : 0);
        std::vector<uint8_t> counted(n_c ? n_c : 1, 0);
        try {
            hc::brr::run_chain(cs, st, min_evidence, found, [&](uint32_t i, int min_ev, std::vector<node_pair_t>& rm) {
                const hc_br_component& C = cs.comps[i];
                const node_pair_t* edges = cs.edges.data() + C.edge_first;
                counted[i] = 1;
                if (C.host_finished & (HC_BR_RED_HOST_NO_ROW | HC_BR_RED_HOST_SHARED_EDGE)) {
                    bool no_row = false;
                    hc::brr::count_unique(lists, edges, C.edge_count, unique.data() + C.edge_first, &no_row);
                    return hc::brr::decide(edges, unique.data() + C.edge_first, C.edge_count, V, min_ev, st->diploid && cs.typical[i], rm);
                }
                if (C.host_finished & HC_BR_RED_HOST_DIPLOID)  // the device's counts, the tie order of a four-entry unordered_map
                    return hc::brr::decide(edges, unique.data() + C.edge_first, C.edge_count, V, min_ev, true, rm);
                for (uint64_t k = 0; k < C.edge_count; k++)
                    if (ce_remove[C.edge_first + k]) rm.push_back(edges[k]);
                return cm_keep[i] != 0;
            });
        } catch (const std::string& what) {
            return fail(me, HC_ERR_ARG, what);
        }
        for (uint64_t i = 0; i < n_c; i++)
            if (!counted[i]) std::fill(unique.begin() + cs.comps[i].edge_first, unique.begin() + cs.comps[i].edge_first + cs.comps[i].edge_count, 0u);
        hc::brr::finish_removals(cs);
        ms_walk += ms_since(t0);
    }
    // 5: the records of edges_to_remove, then the edit
    const uint64_t n_rm = cs.to_remove.size();
    if (n_rm > n_nb) return fail(me, HC_ERR_STATE, "more removals than final_branch edges");
    R.n_rm = n_rm;
    if (n_rm) {
        if ((rc = B.red_pin.ensure(n_rm * 8 + 256))) return rc;
        uint32_t* hu = (uint32_t*)B.red_pin.p;
        uint32_t* hv = hu + n_rm;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t k = 0; k < n_rm; k++) hu[k] = (uint32_t)cs.to_remove[k].first, hv[k] = (uint32_t)cs.to_remove[k].second;
        HC_HIP(hipMemcpyAsync(R.rm_u, hu, n_rm * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(R.rm_v, hv, n_rm * 4, hipMemcpyHostToDevice, s));
        HC_HIP(hipStreamSynchronize(s));
        ms_copy += ms_since(t0);
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hipMemsetAsync(R.counters, 0, hc::br::kRedCounters * 8, s));
        HC_HIP(hc::br::launch_red_find(dg, R, s));
        HC_HIP(hipMemcpyAsync(flags, R.counters, sizeof flags, hipMemcpyDeviceToHost, s));
        if ((rc = timed())) return rc;
        ms_edit += ms;
        if (flags[hc::br::kRedNotFound])
            return fail(me, HC_ERR_ARG, "a pair of edges_to_remove has no record in the graph (the exit(1) of src/BranchReduction.cpp:219-222)");
    }
    HC_HIP(hipEventRecord(c->ev0, s));
    if ((rc = hc::graph_remove_records(c, me, R.rm_rec, R.rm_in, n_rm, B.t_missing.as<hc_edge_rec>(), n_missing))) return rc;
    if ((rc = timed())) return rc;
    ms_edit += ms;
    // the tables of hc_br_reduce_fetch
    B.red_comps = cs.comps;
    B.red_comp_edge.resize(2 * n_ce), B.red_comp_unique.assign(unique.begin(), unique.begin() + n_ce), B.red_removed.resize(2 * n_rm);
    for (uint64_t k = 0; k < n_ce; k++) B.red_comp_edge[2 * k] = (uint32_t)cs.edges[k].first, B.red_comp_edge[2 * k + 1] = (uint32_t)cs.edges[k].second;
    for (uint64_t k = 0; k < n_rm; k++) B.red_removed[2 * k] = (uint32_t)cs.to_remove[k].first, B.red_removed[2 * k + 1] = (uint32_t)cs.to_remove[k].second;
    B.red_valid = true;
    const uint64_t n_items_sorted = counts->n_items_sorted;
    hc::brr::fill_counts(cs, counts);
    counts->n_items_sorted = n_items_sorted;
    counts->n_missing_appended = n_missing;
    counts->ms_device = ms_device, counts->ms_host_walk = ms_walk, counts->ms_copy = ms_copy, counts->ms_sort = ms_sort, counts->ms_edit = ms_edit;
    return HC_OK;
}

int hc_br_reduce_fetch(hc_ctx* c, hc_br_reduce_tables* T) {
    const char* me = "hc_br_reduce_fetch";
    if (!c || !T) return fail(me, HC_ERR_ARG, "null argument");
    const hc_ctx::Br& B = c->br;
    if (!B.red_valid) return fail(me, HC_ERR_STATE, "no tables kept (hc_br_reduce first)");
    const uint64_t n_c = B.red_comps.size(), n_ce = B.red_comp_unique.size(), n_rm = B.red_removed.size() / 2;
    if ((T->components && T->cap_components < n_c) || ((T->comp_edge || T->comp_unique) && T->cap_comp_edges < n_ce) || (T->removed && T->cap_removed < n_rm))
        return fail(me, HC_ERR_ARG, "a table is too small (hc_br_reduce returned the counts)");
    if (T->components && n_c) memcpy(T->components, B.red_comps.data(), n_c * sizeof(hc_br_component));
    if (T->comp_edge && n_ce) memcpy(T->comp_edge, B.red_comp_edge.data(), n_ce * 8);
    if (T->comp_unique && n_ce) memcpy(T->comp_unique, B.red_comp_unique.data(), n_ce * 4);
    if (T->removed && n_rm) memcpy(T->removed, B.red_removed.data(), n_rm * 8);
    return HC_OK;
}

}  // extern "C"
