// hc_api_fno3_resident.cpp — hc_fno3_from_originals / hc_fno3_text_fetch / hc_fno3_candidates_fetch (include/hcsr.h): FNO=3 from the dict
// and the read descriptors the context keeps.  The walk is hc_fno3_walk_kernels.hip around two stable radix sorts, two ordered selections
// and two exclusive sums (hc_prims.hip); from the candidates' records on it is hc_fno3_run's device form (hc_fno_kernels.hip: fno3_deduce,
// fno3_format).  The text and the table are built in blocks of their own and trade places with the kept ones at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_fno3_walk.h"
#include "hc_fno_device.h"
#include "hc_prims.h"

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

}  // namespace

extern "C" {

int hc_fno3_from_originals(hc_ctx* c, const hc_fno3_resident_input* in, hc_fno3_resident_counts* counts) {
    namespace W3 = hc::fno3w;
    const char* me = "hc_fno3_from_originals";
    if (!c || !in || !counts) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    if (!c->have_reads) return fail(me, HC_ERR_STATE, "no read store (hc_set_reads first)");
    hc_ctx::SrOriginals& O = c->sr_orig;
    if (!O.valid) return fail(me, HC_ERR_STATE, "no dict on the device (hc_sr_originals_init or hc_sr_originals_load first)");
    const uint64_t n = c->view.n_reads, ne = O.n_entries;
    if (O.n_reads != n) return fail(me, HC_ERR_STATE, "the kept dict is not over the reads of the store");
    if (const char* what = W3::check_input(in, n)) return fail(me, HC_ERR_ARG, what);
    const uint64_t max_combos = in->max_combos ? in->max_combos : W3::kMaxCombos;
    hc_ctx::SrOriginals::Fno3& F = O.fno3;
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    auto room = [&](hc_scratch& k, size_t bytes) { return k.ensure(bytes ? bytes : 16); };
    using hc::prims::scan_temp_bytes;
    using hc::prims::select_temp_bytes;
    using hc::prims::sort_temp_bytes;
    const size_t temp1 = std::max({sort_temp_bytes(ne ? ne : 1, 8, 4), select_temp_bytes(ne ? ne : 1), scan_temp_bytes(ne + 1, 8)});
    if ((rc = room(F.key1_in, ne * 8)) || (rc = room(F.key1, ne * 8)) || (rc = room(F.val1_in, ne * 4)) || (rc = room(F.val1, ne * 4)) ||
        (rc = room(F.entry_read, ne * 4)) || (rc = room(F.head1, ne)) || (rc = room(F.head1_pos, ne * 4)) || (rc = room(F.cnt, (ne + 1) * 8)) ||
        (rc = room(F.counters, W3::kCounters * 8)) || (rc = room(F.temp, temp1)) || (rc = room(F.rank, in->walk_rank ? n * 4 : 0)))
        return rc;
    W3::Work W{};
    W.key1_in = F.key1_in.as<uint64_t>();
    W.key1 = F.key1.as<uint64_t>();
    W.val1_in = F.val1_in.as<uint32_t>();
    W.val1 = F.val1.as<uint32_t>();
    W.entry_read = F.entry_read.as<uint32_t>();
    W.head1 = F.head1.as<uint8_t>();
    W.head1_pos = F.head1_pos.as<uint32_t>();
    W.cnt = F.cnt.as<uint64_t>();
    W.counters = F.counters.as<unsigned long long>();
    const W3::Dict D{O.off.as<uint64_t>(), O.entries.as<hc_sr_original>(), n, ne};
    if (in->walk_rank) HC_HIP(hipMemcpyAsync(F.rank.p, in->walk_rank, n * 4, hipMemcpyHostToDevice, s));
    const W3::Ranks K{in->walk_rank ? F.rank.as<uint32_t>() : nullptr, in->n_single, in->n_trivial, in->n_paired};
    float ms = 0;
    double ms_device = 0;
    unsigned long long h[W3::kCounters] = {};
    uint64_t n_combos = 0;
    // 1. the entries' keys and the largest id
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hipMemsetAsync(W.counters, 0, W3::kCounters * 8, s));
    if (ne) HC_HIP(W3::launch_keys1(D, K, W, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipMemcpyAsync(h, W.counters, sizeof h, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_device += ms;
    // 2. one run per original, the combinations per entry, their sum
    if (ne) {
        const int end_bit = 32 + W3::bits_for((uint64_t)h[0] + 1);
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::prims::sort_pairs(F.temp.p, F.temp.cap, W.key1_in, W.key1, W.val1_in, W.val1, ne, 0, end_bit, s));
        HC_HIP(W3::launch_heads1(W, ne, s));
        HC_HIP(hc::prims::select_flagged(F.temp.p, F.temp.cap, W.head1, ne, W.head1_pos, W.counters + 1, s));
        HC_HIP(W3::launch_count(W, ne, s));
        HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, W.cnt, W.cnt, ne + 1, s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(h, W.counters, sizeof h, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(&n_combos, W.cnt + ne, 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
    }
    const uint64_t n_originals = h[1];
    counts->n_originals = n_originals;
    counts->n_combos = n_combos;
    counts->ms_device = ms_device;
    if (n_originals > in->original_readcount) {
        F.drop();
        return fail(me, HC_ERR_FORMAT, "the reference stops here: nodes_to_SR.at(index): more originals than original_readcount");
    }
    if (n_combos > max_combos) return fail(me, HC_ERR_NOT_ON_DEVICE, "more (pair, original) combinations than max_combos");
    // 3., 4. the combinations' keys, the stable sort, the candidates and the ambiguous ones
    uint64_t n_cand = 0;
    if (n_combos) {
        const int rank_bits = W3::bits_for(n);
        const size_t temp2 = std::max({sort_temp_bytes(n_combos, 8, 4), select_temp_bytes(n_combos), scan_temp_bytes(n_combos + 1, 4)});
        if ((rc = room(F.key2_in, n_combos * 8)) || (rc = room(F.key2, n_combos * 8)) || (rc = room(F.val2_in, n_combos * 4)) ||
            (rc = room(F.val2, n_combos * 4)) || (rc = room(F.diff, n_combos * sizeof(W3::Diff))) || (rc = room(F.head2, n_combos)) ||
            (rc = room(F.differs, (n_combos + 1) * 4)) || (rc = room(F.head2_pos, n_combos * 4)) || (rc = room(F.temp, temp2)))
            return rc;
        W.key2_in = F.key2_in.as<uint64_t>();
        W.key2 = F.key2.as<uint64_t>();
        W.val2_in = F.val2_in.as<uint32_t>();
        W.val2 = F.val2.as<uint32_t>();
        W.diff = F.diff.as<W3::Diff>();
        W.head2 = F.head2.as<uint8_t>();
        W.differs = F.differs.as<uint32_t>();
        W.head2_pos = F.head2_pos.as<uint32_t>();
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(W3::launch_combos(D, c->d_reads.p, W, n_combos, rank_bits, s));
        HC_HIP(hc::prims::sort_pairs(F.temp.p, F.temp.cap, W.key2_in, W.key2, W.val2_in, W.val2, n_combos, 0, 2 * rank_bits, s));
        HC_HIP(W3::launch_heads2(W, n_combos, s));
        HC_HIP(hc::prims::select_flagged(F.temp.p, F.temp.cap, W.head2, n_combos, W.head2_pos, W.counters + 2, s));
        HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, W.differs, W.differs, n_combos + 1, s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(h, W.counters, sizeof h, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
        n_cand = h[2];
        if (n_cand == 0 || n_cand > n_combos) return fail(me, HC_ERR_STATE, "the selection and the combinations disagree");
    }
    // 5. the candidates' records, then deduceOverlap, the lines' places and the text as hc_fno3_run's device form has them
    uint64_t n_bytes = 0, n_lines = 0, n_ambiguous = 0;
    if ((rc = room(F.next_cands, n_cand * sizeof(hc_fno3_candidate)))) return rc;
    if (n_cand) {
        if ((rc = room(F.items, n_cand * sizeof(hc::FnoItem))) || (rc = room(F.rec, n_cand * sizeof(hc::Fno3Rec))) || (rc = room(F.len, (n_cand + 1) * 8)) ||
            (rc = room(F.off, (n_cand + 1) * 8)) || (rc = room(F.temp, scan_temp_bytes(n_cand + 1, 8))))
            return rc;
        hc::FnoItem* d_items = F.items.as<hc::FnoItem>();
        hc::Fno3Rec* d_rec = F.rec.as<hc::Fno3Rec>();
        uint64_t *d_len = F.len.as<uint64_t>(), *d_off = F.off.as<uint64_t>();
        hc_fno3_candidate* d_cands = F.next_cands.as<hc_fno3_candidate>();
        unsigned long long* d_deduce = W.counters + W3::kDeduceCounters;
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(W3::launch_items(D, c->d_reads.p, W, n_combos, n_cand, d_items, d_cands, s));
        HC_HIP(hc::fno3_deduce(d_items, n_cand, (in->flags & HC_FNO_NO_INCLUSIONS) ? 1u : 0u, d_rec, d_len, d_deduce, s));
        HC_HIP(W3::launch_line_flags(d_len, n_cand, d_cands, s));
        HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, d_len, d_off, n_cand + 1, s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(h, W.counters, sizeof h, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(&n_bytes, d_off + n_cand, 8, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
        counts->candidates = n_cand;
        counts->ms_device = ms_device;
        if (h[W3::kDeduceCounters + 4]) {
            F.drop();
            return fail(me, HC_ERR_FORMAT, "the reference stops here: deduceOverlap (a read of length 0, the assert of :391 or the Overlap constructor's checks)");
        }
        n_lines = h[W3::kDeduceCounters + 5];
        n_ambiguous = h[3];
        if ((rc = room(F.next_text, n_bytes))) return rc;
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::fno3_format(d_rec, d_len, d_off, n_cand, F.next_text.as<char>(), s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_device += ms;
    } else if ((rc = room(F.next_text, 0))) {
        return rc;
    }
    F.text.swap(F.next_text);
    F.cands.swap(F.next_cands);
    F.n_text = n_bytes;
    F.n_cands = n_cand;
    F.valid = true;
    counts->n_lines = n_lines;
    counts->n_bytes = n_bytes;
    counts->candidates = n_cand;
    counts->n_ambiguous = n_ambiguous;
    counts->ms_device = ms_device;
    return HC_OK;
}

int hc_fno3_text_fetch(hc_ctx* c, uint64_t first, uint64_t count, char* dst) {
    const char* me = "hc_fno3_text_fetch";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    const hc_ctx::SrOriginals::Fno3& F = c->sr_orig.fno3;
    if (!F.valid) return fail(me, HC_ERR_STATE, "no text on the device (hc_fno3_from_originals first)");
    if (first > F.n_text || count > F.n_text - first) return fail(me, HC_ERR_ARG, "range beyond the text");
    if (count == 0) return HC_OK;
    if (!dst) return fail(me, HC_ERR_ARG, "null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, F.text.as<char>() + first, count, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

int hc_fno3_candidates_fetch(hc_ctx* c, uint64_t first, uint64_t count, hc_fno3_candidate* dst) {
    const char* me = "hc_fno3_candidates_fetch";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    const hc_ctx::SrOriginals::Fno3& F = c->sr_orig.fno3;
    if (!F.valid) return fail(me, HC_ERR_STATE, "no candidate table on the device (hc_fno3_from_originals first)");
    if (first > F.n_cands || count > F.n_cands - first) return fail(me, HC_ERR_ARG, "range beyond the table");
    if (count == 0) return HC_OK;
    if (!dst) return fail(me, HC_ERR_ARG, "null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, F.cands.as<hc_fno3_candidate>() + first, count * sizeof(hc_fno3_candidate), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

}  // extern "C"
