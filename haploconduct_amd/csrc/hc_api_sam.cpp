// hc_api_sam.cpp — hc_set_sam_records, hc_sam_plan, hc_sam_lines_device, hc_sam_lines_fetch, hc_sam_plan_counts (include/hcedge.h):
// scripts/sam2overlaps.py's enumeration of reference-guided overlaps on the device (kernels: hc_sam_kernels.hip; one pair: hc_sam_items.h).
// The upload validates what the kernels index with and what the sort key holds; everything the device does not decide — and every record on
// which the host mirror (host/Sam2Overlaps.cpp) would report a status — is HC_ERR_NOT_ON_DEVICE, never a wrong line.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sam.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {
const uint64_t kWindowPerCandidate = 64;  // a wave's step: a window up to 64 records per evaluated pair (and record) costs no step more

hc::SamSorted sorted_view(const hc_ctx::Sam& M) {
    return hc::SamSorted{M.pos.as<int32_t>(), M.len.as<uint32_t>(), M.ref.as<uint32_t>(), M.rec.as<hc_sam_rec>(), M.n_recs};
}
}  // namespace

extern "C" int hc_set_sam_records(hc_ctx* c, const hc_sam_aln* alns, uint64_t n_alns, const hc_sam_rec* recs, uint64_t n_recs, const hc_sam_op* ops,
                                  uint64_t n_ops, const uint64_t* ref_len, uint64_t n_refs) {
    const char* me = "hc_set_sam_records: ";
    if (!c) return fail(HC_ERR_ARG, std::string(me) + "null context");
    if ((n_alns && !alns) || (n_recs && !recs) || (n_ops && !ops) || (n_refs && !ref_len)) return fail(HC_ERR_ARG, std::string(me) + "an array is missing");
    hc_ctx::Sam& M = c->sam;
    auto not_here = [&](const char* why) { return fail(HC_ERR_NOT_ON_DEVICE, std::string(me) + "not on the device (" + why + ")"); };
    if (n_recs == 0) return not_here("no record: the script exits");
    if (n_recs >= (1ull << 31) || n_alns >= (1ull << 31) || n_ops >= (1ull << 32) || n_refs >= (1ull << 30) || n_refs == 0)
        return not_here("more records, operations or references than the sort key holds");
    const int64_t lim = 1ll << 30;
    for (uint64_t a = 0; a < n_alns; a++) {
        const hc_sam_aln& x = alns[a];
        if ((uint64_t)x.op_first + x.op_count > n_ops) return fail(HC_ERR_ARG, std::string(me) + "an alignment's operations lie outside the array");
        if (!(x.marks & HC_SAM_ID_PLAIN)) return not_here("an id that is not a plain decimal");
        if (!(x.marks & HC_SAM_CIGAR_PLAIN) || x.op_count == 0) return not_here("a CIGAR that is not ([0-9]+[A-Z=])+");
        if (x.cpos <= -lim || x.cpos >= lim || x.len >= (uint64_t)lim) return not_here("a position or length of 2^30 and more");
        uint64_t sum = 0;
        for (uint32_t k = 0; k < x.op_count; k++) {
            const hc_sam_op& o = ops[x.op_first + k];
            if (o.count == 0 || !((o.letter >= 'A' && o.letter <= 'Z') || o.letter == '=')) return not_here("a CIGAR that is not ([0-9]+[A-Z=])+");
            sum += o.count;
        }
        if (sum >= (uint64_t)lim) return not_here("a CIGAR that spans 2^30 bases and more");
    }
    std::vector<uint32_t> seg(n_refs + 1, 0);
    for (uint64_t k = 0; k < n_recs; k++) {
        const hc_sam_rec& r = recs[k];
        if (r.first >= n_alns || (r.second != HC_SAM_NONE && r.second >= n_alns)) return fail(HC_ERR_ARG, std::string(me) + "a record points outside the alignments");
        if (alns[r.first].ref >= n_refs) return fail(HC_ERR_ARG, std::string(me) + "a record of no reference");
        if (r.second != HC_SAM_NONE && alns[r.second].len == 0) return not_here("a second mate of length 0: the script divides by it");
        seg[alns[r.first].ref + 1]++;
    }
    for (uint64_t r = 0; r < n_refs; r++) seg[r + 1] += seg[r];
    HC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc;
    M.loaded = M.planned = false;
    if ((rc = M.alns.ensure(std::max<uint64_t>(n_alns, 1) * sizeof(hc_sam_aln))) || (rc = M.recs.ensure(n_recs * sizeof(hc_sam_rec))) ||
        (rc = M.ops.ensure(std::max<uint64_t>(n_ops, 1) * sizeof(hc_sam_op))) || (rc = M.ref_len.ensure(n_refs * sizeof(uint64_t))) ||
        (rc = M.seg_begin.ensure((n_refs + 1) * sizeof(uint32_t))) || (rc = M.proc_end.ensure(n_refs * sizeof(uint32_t))))
        return rc;
    HC_HIP(hipMemcpyAsync(M.alns.p, alns, n_alns * sizeof(hc_sam_aln), hipMemcpyHostToDevice, st));
    HC_HIP(hipMemcpyAsync(M.recs.p, recs, n_recs * sizeof(hc_sam_rec), hipMemcpyHostToDevice, st));
    if (n_ops) HC_HIP(hipMemcpyAsync(M.ops.p, ops, n_ops * sizeof(hc_sam_op), hipMemcpyHostToDevice, st));
    HC_HIP(hipMemcpyAsync(M.ref_len.p, ref_len, n_refs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HC_HIP(hipMemcpyAsync(M.seg_begin.p, seg.data(), seg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HC_HIP(hipStreamSynchronize(st));  // (the caller's arrays and `seg` are pageable: nothing of them is read after this call)
    M.n_alns = (uint32_t)n_alns, M.n_recs = (uint32_t)n_recs, M.n_refs = (uint32_t)n_refs, M.n_ops = n_ops;
    M.key_bits = 32;
    while (M.key_bits < 64 && (n_refs >> (M.key_bits - 32))) M.key_bits++;
    M.loaded = true;
    return HC_OK;
}

extern "C" int hc_sam_plan(hc_ctx* c, int64_t min_overlap_len, uint64_t* n_lines) {
    const char* me = "hc_sam_plan: ";
    if (!c || !n_lines) return fail(HC_ERR_ARG, std::string(me) + "null argument");
    hc_ctx::Sam& M = c->sam;
    if (!M.loaded) return fail(HC_ERR_STATE, std::string(me) + "no records (hc_set_sam_records)");
    if (min_overlap_len <= -(1ll << 31) || min_overlap_len >= (1ll << 31))
        return fail(HC_ERR_NOT_ON_DEVICE, std::string(me) + "not on the device (min_overlap_len beyond 32 bits)");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const uint32_t n = M.n_recs;
    M.planned = false;
    int rc;
    const size_t sort_bytes = hc::prims::sort_temp_bytes(n, sizeof(uint64_t), sizeof(uint32_t));
    const size_t scan_bytes = hc::prims::scan_temp_bytes((uint64_t)n + 1, sizeof(uint64_t));
    const uint32_t tiles = (n + 1023) / 1024;
    if ((rc = M.keys.ensure((size_t)n * 8)) || (rc = M.keys_out.ensure((size_t)n * 8)) || (rc = M.iota.ensure((size_t)n * 4)) ||
        (rc = M.perm.ensure((size_t)n * 4)) || (rc = M.cnt.ensure(((size_t)n + 1) * 8)) || (rc = M.temp.ensure(std::max<size_t>(std::max(sort_bytes, scan_bytes), 16))) ||
        (rc = M.pmax.ensure((size_t)n * 4)) || (rc = M.tiles.ensure((size_t)tiles * 4)) || (rc = M.status.ensure(sizeof(unsigned long long))) ||
        (rc = M.range.ensure(2 * sizeof(uint32_t))) || (rc = M.pos.ensure((size_t)n * 4)) || (rc = M.len.ensure((size_t)n * 4)) ||
        (rc = M.ref.ensure((size_t)n * 4)) || (rc = M.rec.ensure((size_t)n * sizeof(hc_sam_rec))) || (rc = M.e.ensure((size_t)n * 4)) ||
        (rc = M.lo.ensure((size_t)n * 4)) || (rc = M.off.ensure(((size_t)n + 1) * 8)))
        return rc;
    const hc_sam_aln* alns = M.alns.as<hc_sam_aln>();
    const hc_sam_op* ops = M.ops.as<hc_sam_op>();
    uint64_t* cnt = M.cnt.as<uint64_t>();
    uint64_t* off = M.off.as<uint64_t>();
    // the script's order: one stable sort by (reference, biased position, kind); input order breaks the ties
    HC_HIP(hc::sam_keys(alns, M.recs.as<hc_sam_rec>(), n, M.keys.as<uint64_t>(), M.iota.as<uint32_t>(), st));
    HC_HIP(hc::prims::sort_pairs(M.temp.p, M.temp.cap, M.keys.as<uint64_t>(), M.keys_out.as<uint64_t>(), M.iota.as<uint32_t>(), M.perm.as<uint32_t>(), n, 0,
                                 M.key_bits, st));
    HC_HIP(hc::sam_gather(alns, M.recs.as<hc_sam_rec>(), M.perm.as<uint32_t>(), n, M.pos.as<int32_t>(), M.len.as<uint32_t>(), M.ref.as<uint32_t>(),
                          M.rec.as<hc_sam_rec>(), st));
    const hc::SamSorted S = sorted_view(M);
    HC_HIP(hc::sam_processed(S.pos, M.seg_begin.as<uint32_t>(), M.ref_len.as<uint64_t>(), M.n_refs, M.proc_end.as<uint32_t>(), st));
    // per j its last partner e_j; the candidates' sum
    HC_HIP(hipMemsetAsync(cnt + n, 0, sizeof(uint64_t), st));
    HC_HIP(hc::sam_last_partner(S, M.seg_begin.as<uint32_t>(), M.proc_end.as<uint32_t>(), min_overlap_len, M.e.as<uint32_t>(), cnt, st));
    HC_HIP(hc::prims::exclusive_sum(M.temp.p, M.temp.cap, cnt, off, (uint64_t)n + 1, st));
    uint64_t totals[2] = {0, 0};
    HC_HIP(hipMemcpyAsync(&totals[0], off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    // per i the lowest j that can still be active; the windows' sum
    HC_HIP(hc::sam_prefix_max(M.e.as<uint32_t>(), n, M.pmax.as<uint32_t>(), M.tiles.as<uint32_t>(), st));
    HC_HIP(hc::sam_window(S, M.seg_begin.as<uint32_t>(), M.proc_end.as<uint32_t>(), M.pmax.as<uint32_t>(), M.lo.as<uint32_t>(), cnt, st));
    HC_HIP(hc::prims::exclusive_sum(M.temp.p, M.temp.cap, cnt, off, (uint64_t)n + 1, st));
    HC_HIP(hipMemcpyAsync(&totals[1], off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
    M.n_candidates = totals[0];
    M.n_window = totals[1];
    if (M.n_window > kWindowPerCandidate * (M.n_candidates + n))
        return fail(HC_ERR_NOT_ON_DEVICE, std::string(me) + "not on the device (the windows hold " + std::to_string(M.n_window) + " records for " +
                                              std::to_string(M.n_candidates) + " evaluated pairs: a long read among short ones)");
    // the count pass and the one exclusive sum that stays
    unsigned long long* d_status = M.status.as<unsigned long long>();
    HC_HIP(hipMemsetAsync(d_status, 0, sizeof(unsigned long long), st));
    HC_HIP(hc::sam_count(S, alns, ops, M.lo.as<uint32_t>(), M.e.as<uint32_t>(), min_overlap_len, cnt, d_status, st));
    HC_HIP(hc::prims::exclusive_sum(M.temp.p, M.temp.cap, cnt, off, (uint64_t)n + 1, st));
    unsigned long long status = 0;
    uint64_t lines = 0;
    HC_HIP(hipMemcpyAsync(&status, d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HC_HIP(hipMemcpyAsync(&lines, off + n, sizeof lines, hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
    if (status)
        return fail(HC_ERR_NOT_ON_DEVICE, std::string(me) + "not on the device (" +
                                              (status & hc::kSamStatusScript ? "a pair on which the script dies" : "a number an overlap line does not hold") + ")");
    M.mol = min_overlap_len;
    M.n_lines = lines;
    M.planned = true;
    *n_lines = lines;
    return HC_OK;
}

extern "C" int hc_sam_lines_device(hc_ctx* c, uint64_t first_line, uint64_t n, hc_line_rec* d_lines) {
    const char* me = "hc_sam_lines_device: ";
    if (!c) return fail(HC_ERR_ARG, std::string(me) + "null context");
    hc_ctx::Sam& M = c->sam;
    if (!M.planned) return fail(HC_ERR_STATE, std::string(me) + "no plan (hc_sam_plan)");
    if (first_line > M.n_lines || n > M.n_lines - first_line) return fail(HC_ERR_ARG, std::string(me) + "lines beyond the file's end");
    if (n == 0) return HC_OK;
    if (!d_lines) return fail(HC_ERR_ARG, std::string(me) + "null destination");
    HC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    uint32_t range[2] = {0, 0};
    HC_HIP(hc::sam_owner_range(M.off.as<uint64_t>(), M.n_recs, first_line, n, M.range.as<uint32_t>(), st));
    HC_HIP(hipMemcpyAsync(range, M.range.p, sizeof range, hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
    if (range[0] > range[1] || range[1] > M.n_recs) return fail(HC_ERR_STATE, std::string(me) + "the owners of the lines lie outside the records");
    HC_HIP(hc::sam_write(sorted_view(M), M.alns.as<hc_sam_aln>(), M.ops.as<hc_sam_op>(), M.lo.as<uint32_t>(), M.e.as<uint32_t>(), M.off.as<uint64_t>(), M.mol,
                         range[0], range[1], first_line, n, d_lines, st));
    HC_HIP(hipStreamSynchronize(st));
    return HC_OK;
}

extern "C" int hc_sam_lines_fetch(hc_ctx* c, uint64_t first_line, uint64_t n, hc_line_rec* out) {
    const char* me = "hc_sam_lines_fetch: ";
    if (!c) return fail(HC_ERR_ARG, std::string(me) + "null context");
    if (n == 0) return c->sam.planned ? HC_OK : fail(HC_ERR_STATE, std::string(me) + "no plan (hc_sam_plan)");
    if (!out) return fail(HC_ERR_ARG, std::string(me) + "null destination");
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::Sam& M = c->sam;
    const uint64_t piece = 1ull << 20;  // 48 MB of lines at a time
    int rc;
    if ((rc = M.stage.ensure(std::min(n, piece) * sizeof(hc_line_rec)))) return rc;
    for (uint64_t at = 0; at < n; at += piece) {
        const uint64_t k = std::min(piece, n - at);
        if ((rc = hc_sam_lines_device(c, first_line + at, k, M.stage.as<hc_line_rec>()))) return rc;
        HC_HIP(hipMemcpy(out + at, M.stage.p, k * sizeof(hc_line_rec), hipMemcpyDeviceToHost));
    }
    return HC_OK;
}

extern "C" int hc_sam_lines_slot(hc_ctx* c, uint32_t slot, uint64_t first_line, uint64_t n, const hc_line_rec** d_lines) {
    if (!c || !d_lines) return fail(HC_ERR_ARG, "hc_sam_lines_slot: null argument");
    if (slot >= 16) return fail(HC_ERR_ARG, "hc_sam_lines_slot: slots are 0 .. 15");
    HC_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = c->sam.slot[slot].ensure(std::max<uint64_t>(n, 1) * sizeof(hc_line_rec)))) return rc;
    if ((rc = hc_sam_lines_device(c, first_line, n, c->sam.slot[slot].as<hc_line_rec>()))) return rc;
    *d_lines = c->sam.slot[slot].as<hc_line_rec>();
    return HC_OK;
}

extern "C" int hc_sam_plan_counts(hc_ctx* c, uint64_t* n_candidates, uint64_t* n_window) {
    if (!c) return fail(HC_ERR_ARG, "hc_sam_plan_counts: null context");
    if (n_candidates) *n_candidates = c->sam.n_candidates;
    if (n_window) *n_window = c->sam.n_window;
    return HC_OK;
}
