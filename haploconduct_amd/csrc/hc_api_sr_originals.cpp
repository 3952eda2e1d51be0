// hc_api_sr_originals.cpp — hc_sr_originals_init / _load / _fetch / _next / _write_text / _text_fetch (include/hcsr.h): the original-read
// index maps (OverlapGraph::original_ID_dict) as a CSR kept in the context, the next store's built from the current one's by the kernels of
// hc_sr_originals_kernels.hip around one exclusive sum, one stable radix sort and one ordered selection (hc_prims.hip), and the bytes of
// subreads.txt.  The new dict is built in blocks of its own and trades places with the kept one at the end: any error leaves the old one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr_originals.h"

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

int bits_for(uint64_t n) {  // bits that hold every value below n
    int b = 1;
    while (b < 32 && (1ull << b) < n) b++;
    return b;
}

}  // namespace

extern "C" {

int hc_sr_originals_init(hc_ctx* c) {
    const char* me = "hc_sr_originals_init";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    if (!c->have_reads) return fail(me, HC_ERR_STATE, "no read store (hc_set_reads first)");
    hc_ctx::SrOriginals& O = c->sr_orig;
    const uint32_t n = c->view.n_reads;
    HC_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = O.next_off.ensure(((uint64_t)n + 1) * 8)) || (rc = O.next_entries.ensure((n ? n : 1) * sizeof(hc_sr_original)))) return rc;
    HC_HIP(hc::orig::launch_init(c->d_reads.p, n, O.next_off.as<uint64_t>(), O.next_entries.as<hc_sr_original>(), c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    O.off.swap(O.next_off);
    O.entries.swap(O.next_entries);
    O.n_reads = O.n_entries = n;
    O.valid = true;
    O.replaced();
    return HC_OK;
}

int hc_sr_originals_load(hc_ctx* c, const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads) {
    const char* me = "hc_sr_originals_load";
    if (!c || !orig_off) return fail(me, HC_ERR_ARG, "null argument");
    if (!c->have_reads) return fail(me, HC_ERR_STATE, "no read store (hc_set_reads first)");
    if (n_reads != c->view.n_reads) return fail(me, HC_ERR_ARG, "n_reads is not the number of reads of the current store");
    if (const char* what = hc::orig::check_dict(orig_off, entries, n_reads)) return fail(me, HC_ERR_ARG, what);
    const uint64_t ne = orig_off[n_reads];
    std::vector<hc_sr_original> clean(entries, entries + ne);
    for (hc_sr_original& e : clean) {
        if (!e.paired) e.index2 = 0, e.len2 = 0;
        e.pad[0] = e.pad[1] = 0;
    }
    hc_ctx::SrOriginals& O = c->sr_orig;
    HC_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = O.next_off.ensure((n_reads + 1) * 8)) || (rc = O.next_entries.ensure((ne ? ne : 1) * sizeof(hc_sr_original)))) return rc;
    HC_HIP(hipMemcpyAsync(O.next_off.p, orig_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (ne) HC_HIP(hipMemcpyAsync(O.next_entries.p, clean.data(), ne * sizeof(hc_sr_original), hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    O.off.swap(O.next_off);
    O.entries.swap(O.next_entries);
    O.n_reads = n_reads;
    O.n_entries = ne;
    O.valid = true;
    O.replaced();
    return HC_OK;
}

int hc_sr_originals_fetch(hc_ctx* c, uint64_t* orig_off, uint64_t cap_reads, hc_sr_original* entries, uint64_t cap_entries, uint64_t* n_reads,
                          uint64_t* n_entries) {
    const char* me = "hc_sr_originals_fetch";
    if (!c || !n_reads || !n_entries) return fail(me, HC_ERR_ARG, "null argument");
    const hc_ctx::SrOriginals& O = c->sr_orig;
    *n_reads = O.valid ? O.n_reads : 0;
    *n_entries = O.valid ? O.n_entries : 0;
    if (!O.valid) return fail(me, HC_ERR_STATE, "no dict on the device (hc_sr_originals_init or hc_sr_originals_load first)");
    if (!orig_off || cap_reads < O.n_reads || cap_entries < O.n_entries || (O.n_entries && !entries))
        return fail(me, HC_ERR_ARG, "a buffer is missing or too small (the sizes are filled)");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(orig_off, O.off.p, (O.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (O.n_entries) HC_HIP(hipMemcpyAsync(entries, O.entries.p, O.n_entries * sizeof(hc_sr_original), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

int hc_sr_originals_next(hc_ctx* c, const hc_sr_originals_input* in, hc_sr_originals_output* out) {
    const char* me = "hc_sr_originals_next";
    if (!c || !in || !out) return fail(me, HC_ERR_ARG, "null argument");
    hc_ctx::SrOriginals& O = c->sr_orig;
    out->n_entries = out->n_failed = 0;
    out->ms_device = out->ms_copy = 0;
    if (!O.valid) return fail(me, HC_ERR_STATE, "no dict on the device (hc_sr_originals_init or hc_sr_originals_load first)");
    if (const char* what = hc::orig::check_input(in, out, nullptr, O.n_reads, nullptr)) return fail(me, HC_ERR_ARG, what);
    const uint64_t nc = in->n_cliques, ns = in->n_srs, nv = in->n_vertices, n_new = in->new_read_count;
    const uint64_t n_sub = ns ? in->subread_off[ns] : 0, n_src = n_sub + nv, n_layouts = nc ? in->first_layout[nc] : 0;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    auto room = [&](hc_scratch& k, size_t bytes) { return k.ensure(bytes ? bytes : 16); };
    if ((rc = room(O.in_kind, nc * 4)) || (rc = room(O.in_new_id, nc * 4)) || (rc = room(O.in_overlap_pos, nc * 4)) ||
        (rc = room(O.in_first_layout, (nc + 1) * 8)) || (rc = room(O.in_layouts, n_layouts * sizeof(hc_sr_layout))) || (rc = room(O.in_sr_clique, ns * 4)) ||
        (rc = room(O.in_subread_off, (ns + 1) * 8)) || (rc = room(O.in_subreads, n_sub * sizeof(hc_fno_subread))) || (rc = room(O.in_vertex_state, nv * 4)) ||
        (rc = room(O.in_nodes, nv * sizeof(hc_fno_read))) || (rc = room(O.in_vertex_read, nv * 4)) || (rc = room(O.in_vertex_fwd, nv)) ||
        (rc = room(O.cnt, (n_src + 1) * 8)) || (rc = room(O.cnt_off, (n_src + 1) * 8)) || (rc = room(O.bits, n_new * 4)) || (rc = room(O.n_sel, 8)) ||
        (rc = room(O.out_status, n_new * 4)) || (rc = room(O.next_off, (n_new + 1) * 8)) ||
        (rc = room(O.temp, hc::prims::scan_temp_bytes(n_src + 1, sizeof(uint64_t)))))
        return rc;
    const auto t_up = std::chrono::steady_clock::now();
    auto up = [&](hc_scratch& k, const void* p, size_t bytes) { return bytes ? hipMemcpyAsync(k.p, p, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    const uint64_t zero_off[1] = {0};
    HC_HIP(up(O.in_kind, in->kind, nc * 4));
    HC_HIP(up(O.in_new_id, in->new_id, nc * 4));
    HC_HIP(up(O.in_overlap_pos, in->overlap_pos, nc * 4));
    HC_HIP(up(O.in_first_layout, nc ? in->first_layout : zero_off, (nc + 1) * 8));
    HC_HIP(up(O.in_layouts, in->layouts, n_layouts * sizeof(hc_sr_layout)));
    HC_HIP(up(O.in_sr_clique, in->sr_clique, ns * 4));
    HC_HIP(up(O.in_subread_off, ns ? in->subread_off : zero_off, (ns + 1) * 8));
    HC_HIP(up(O.in_subreads, in->subreads, n_sub * sizeof(hc_fno_subread)));
    HC_HIP(up(O.in_vertex_state, in->vertex_state, nv * 4));
    HC_HIP(up(O.in_nodes, in->nodes, nv * sizeof(hc_fno_read)));
    HC_HIP(up(O.in_vertex_read, in->vertex_read, nv * 4));
    HC_HIP(up(O.in_vertex_fwd, in->vertex_fwd, nv));
    HC_HIP(hipStreamSynchronize(s));
    double ms_copy = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    hc::orig::In I{O.in_kind.as<uint32_t>(), O.in_new_id.as<int32_t>(), O.in_overlap_pos.as<int32_t>(), O.in_first_layout.as<uint64_t>(),
                   O.in_layouts.as<hc_sr_layout>(), O.in_sr_clique.as<uint32_t>(), O.in_subread_off.as<uint64_t>(), O.in_subreads.as<hc_fno_subread>(),
                   O.in_vertex_state.as<uint32_t>(), O.in_nodes.as<hc_fno_read>(), O.in_vertex_read.as<uint32_t>(), O.in_vertex_fwd.as<uint8_t>(),
                   nc, ns, n_sub, nv, n_new, in->first_it};
    const hc::orig::Dict D{O.off.as<uint64_t>(), O.entries.as<hc_sr_original>(), O.n_reads, O.n_entries};
    hc::orig::Work W{};
    W.cnt = O.cnt.as<uint64_t>();
    W.cnt_off = O.cnt_off.as<uint64_t>();
    W.bits = O.bits.as<uint32_t>();
    W.n_sel = O.n_sel.as<unsigned long long>();
    W.out_off = O.next_off.as<uint64_t>();
    W.out_status = O.out_status.as<uint32_t>();
    float ms = 0;
    double ms_device = 0;
    // 1., 2. the sources' dict lengths and their sum
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hipMemsetAsync(W.bits, 0, (n_new ? n_new : 1) * 4, s));
    HC_HIP(hipMemsetAsync(W.n_sel, 0, 8, s));
    HC_HIP(hc::orig::launch_count(I, D, W, s));
    HC_HIP(hc::prims::exclusive_sum(O.temp.p, O.temp.cap, W.cnt, W.cnt_off, n_src + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t n_cand = 0;
    HC_HIP(hipMemcpyAsync(&n_cand, W.cnt_off + n_src, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    if (n_cand >= (1ull << 31)) return fail(me, HC_ERR_ARG, "2^31 candidate entries or more");
    const int end_bit = 32 + bits_for(n_new);
    const size_t temp_bytes = std::max({hc::prims::sort_temp_bytes(n_cand ? n_cand : 1, sizeof(uint64_t), sizeof(uint32_t)),
                                        hc::prims::select_temp_bytes(n_cand ? n_cand : 1), hc::prims::scan_temp_bytes(n_src + 1, sizeof(uint64_t))});
    if ((rc = room(O.key_in, n_cand * 8)) || (rc = room(O.key, n_cand * 8)) || (rc = room(O.val_in, n_cand * 4)) || (rc = room(O.val, n_cand * 4)) ||
        (rc = room(O.cand, n_cand * sizeof(hc_sr_original))) || (rc = room(O.flag, n_cand)) || (rc = room(O.sel, n_cand * 4)) ||
        (rc = room(O.out_id, n_cand * 4)) || (rc = room(O.next_entries, n_cand * sizeof(hc_sr_original))) || (rc = room(O.temp, temp_bytes)))
        return rc;
    W.key_in = O.key_in.as<uint64_t>();
    W.key = O.key.as<uint64_t>();
    W.val_in = O.val_in.as<uint32_t>();
    W.val = O.val.as<uint32_t>();
    W.cand = O.cand.as<hc_sr_original>();
    W.flag = O.flag.as<uint8_t>();
    W.sel = O.sel.as<uint32_t>();
    W.out_id = O.out_id.as<uint32_t>();
    W.out_entries = O.next_entries.as<hc_sr_original>();
    // 3. - 5. the candidates, the sort, the winners, the selection, the gather, the offsets
    HC_HIP(hipEventRecord(c->ev0, s));
    if (n_cand) {
        HC_HIP(hc::orig::launch_candidates(I, D, W, n_cand, s));
        HC_HIP(hc::prims::sort_pairs(O.temp.p, O.temp.cap, W.key_in, W.key, W.val_in, W.val, n_cand, 0, end_bit, s));
        HC_HIP(hc::orig::launch_first(W, n_cand, s));
        HC_HIP(hc::orig::launch_keep(W, n_cand, s));
        HC_HIP(hc::prims::select_flagged(O.temp.p, O.temp.cap, W.flag, n_cand, W.sel, W.n_sel, s));
        HC_HIP(hc::orig::launch_gather(W, n_cand, s));
    }
    HC_HIP(hc::orig::launch_offsets(I, W, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipEventSynchronize(c->ev1));  // (ms_copy is the copies' own wait, not the kernels')
    const auto t_down = std::chrono::steady_clock::now();
    unsigned long long n_out = 0;
    HC_HIP(hipMemcpyAsync(&n_out, W.n_sel, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(out->orig_off, W.out_off, (n_new + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n_new) HC_HIP(hipMemcpyAsync(out->status, W.out_status, n_new * 4, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    ms_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    if (n_out > n_cand || out->orig_off[n_new] != n_out) return fail(me, HC_ERR_STATE, "the selection and the offsets disagree");
    uint64_t n_failed = 0;
    for (uint64_t r = 0; r < n_new; r++) n_failed += out->status[r] != HC_SR_ORIG_OK;
    O.off.swap(O.next_off);
    O.entries.swap(O.next_entries);
    O.n_reads = n_new;
    O.n_entries = n_out;
    O.replaced();
    out->n_entries = n_out;
    out->n_failed = n_failed;
    out->ms_device = ms_device;
    out->ms_copy = ms_copy;
    return n_failed ? HC_SR_ORIG_SOME_FAILED : HC_OK;
}

int hc_sr_originals_write_text(hc_ctx* c, hc_sr_originals_text_counts* counts) {
    const char* me = "hc_sr_originals_write_text";
    if (!c || !counts) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::SrOriginals& O = c->sr_orig;
    O.text_replaced();
    if (!O.valid) return fail(me, HC_ERR_STATE, "no dict on the device (hc_sr_originals_init or hc_sr_originals_load first)");
    const uint64_t n_items = O.n_entries + O.n_reads;
    if (n_items + 1 >= (1ull << 32)) return fail(me, HC_ERR_ARG, "2^32 items or more");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    if ((rc = O.sizes.ensure((n_items + 1) * 8)) || (rc = O.temp.ensure(hc::prims::scan_temp_bytes(n_items + 1, sizeof(uint64_t))))) return rc;
    const hc::orig::Dict D{O.off.as<uint64_t>(), O.entries.as<hc_sr_original>(), O.n_reads, O.n_entries};
    uint64_t* d_sizes = O.sizes.as<uint64_t>();
    float ms = 0;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::orig::launch_text_sizes(D, d_sizes, s));
    HC_HIP(hc::prims::exclusive_sum(O.temp.p, O.temp.cap, d_sizes, d_sizes, n_items + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t n_bytes = 0;
    HC_HIP(hipMemcpyAsync(&n_bytes, d_sizes + n_items, 8, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device = ms;
    if ((rc = O.text.ensure(n_bytes ? n_bytes : 1))) return rc;
    HC_HIP(hipEventRecord(c->ev0, s));
    if (n_items) HC_HIP(hc::orig::launch_text_write(D, d_sizes, O.text.as<char>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device += ms;
    counts->n_bytes = n_bytes;
    counts->n_lines = O.n_reads;
    O.n_text = n_bytes;
    O.text_valid = true;
    return HC_OK;
}

int hc_sr_originals_text_fetch(hc_ctx* c, uint64_t first, uint64_t count, char* dst) {
    const char* me = "hc_sr_originals_text_fetch";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    const hc_ctx::SrOriginals& O = c->sr_orig;
    if (!O.text_valid) return fail(me, HC_ERR_STATE, "no text on the device (hc_sr_originals_write_text first)");
    if (first > O.n_text || count > O.n_text - first) return fail(me, HC_ERR_ARG, "range beyond the text");
    if (count == 0) return HC_OK;
    if (!dst) return fail(me, HC_ERR_ARG, "null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, O.text.as<char>() + first, count, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

}  // extern "C"
