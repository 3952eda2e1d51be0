// hc_api_sr_next.cpp — hc_sr_keep_device, hc_sr_set_next_reads and hc_sr_next_reads_fetch (include/hcsr.h): the next iteration's read
// store from the kept consensus bytes, the call's extra bytes and the kept raw arrays of the current store.  The kernels of
// hc_sr_next_kernels.hip test, number and gather on the device; the byte histograms, the new offsets and the statuses come back, the
// host plans as hc_set_reads does (hc_api.cpp: plan_store) and the encoder runs on the new raw arrays where they lie (finish_store).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr_merge_next.h"
#include "hc_sr_next.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

extern "C" int hc_sr_keep_device(hc_ctx* c, int on) {
    if (!c) return fail(HC_ERR_ARG, "hc_sr_keep_device: null context");
    hc_ctx::SrNext& N = c->srn;
    N.keep = on != 0;
    if (!N.keep) {  // what was kept goes; the consensus call's own scratch stays its own
        HC_HIP(hipSetDevice(c->device));
        HC_HIP(hipStreamSynchronize(c->stream));
        for (hc_scratch* b : {&N.bases, &N.quals, &N.off, &N.first, &N.next_bases, &N.next_quals, &N.next_off, &N.next_first, &N.entries, &N.status,
                              &N.cnt, &N.bytes, &N.cnt_off, &N.byte_off, &N.temp, &N.hist, &N.extra_seq, &N.extra_qual, &c->sr.patches})
            b->release();
        N.raw_valid = false;
        N.total = 0;
        N.prev_clear();
        c->sr_fastq.drop();
        N.h_off.clear();
        N.h_first.clear();
        c->sr.kept_valid = false;
        c->sr.kept_bytes = 0;
    }
    return HC_OK;
}

// From "the entries, their statuses and the two sums are on the device" on: the survivors' bytes are gathered, the host plans as
// hc_set_reads does and the encoder runs on the new raw arrays.  hc_sr_set_next_reads and hc_sr_merge_next both end here.
int hc::sr_next_store(hc_ctx* c, uint64_t n, uint64_t n_extra, uint32_t n_kept, uint32_t n_seq, uint64_t total, hc_sr_next_counts& cn) {
    hc_ctx::SrNext& N = c->srn;
    hipStream_t s = c->stream;
    const uint32_t n_reads_old = (uint32_t)(N.h_first.size() - 1);
    const hc::SrNextSources S{c->sr.kept_valid ? c->sr.kept_bytes : 0, n_extra, N.off.as<uint64_t>(), N.first.as<uint32_t>(), n_reads_old};
    const hc::SrNextBytes B{{c->sr.seq.as<uint8_t>(), N.extra_seq.as<uint8_t>(), N.bases.as<uint8_t>()},
                            {c->sr.qual.as<uint8_t>(), N.extra_qual.as<uint8_t>(), N.quals.as<uint8_t>()}};
    int rc;
    float ms_b = 0;
    if ((rc = N.hist.ensure(512 * sizeof(unsigned long long)))) return rc;
    N.prev_clear();  // the next_* blocks are about to be overwritten: whatever store they held is gone, and a FASTQ text made from it
    c->sr_fastq.drop();
    const uint32_t n_seq_old = (uint32_t)(N.h_off.size() - 1);
    const uint64_t total_old = N.total;
    // the survivors' bytes, the new offsets and the byte histograms
    if ((rc = N.next_bases.ensure_exact(total)) || (rc = N.next_quals.ensure_exact(total)) ||
        (rc = N.next_off.ensure_exact(sizeof(uint64_t) * ((size_t)n_seq + 1))) || (rc = N.next_first.ensure_exact(sizeof(uint32_t) * ((size_t)n_kept + 1))))
        return rc;
    HC_HIP(hipMemsetAsync(N.hist.p, 0, 512 * sizeof(unsigned long long), s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_next_launch_gather(N.entries.as<hc_sr_next_entry>(), n, S, B, N.status.as<uint32_t>(), N.cnt_off.as<uint64_t>(),
                                     N.byte_off.as<uint64_t>(), N.next_bases.as<uint8_t>(), N.next_quals.as<uint8_t>(), N.next_off.as<uint64_t>(),
                                     N.next_first.as<uint32_t>(), s));
    HC_HIP(hc::sr_next_launch_hist(N.next_bases.as<uint8_t>(), N.next_quals.as<uint8_t>(), total, c->n_cu, N.hist.as<unsigned long long>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    std::vector<uint64_t> h_off((size_t)n_seq + 1);
    std::vector<uint32_t> h_first((size_t)n_kept + 1);
    unsigned long long hist[512];
    HC_HIP(hipMemcpyAsync(h_off.data(), N.next_off.p, h_off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(h_first.data(), N.next_first.p, h_first.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(hist, N.hist.p, sizeof hist, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_b, c->ev0, c->ev1));
    const auto t0 = std::chrono::steady_clock::now();
    hc::StorePlan P;
    P.seq_len.resize(n_seq);
    for (uint32_t q = 0; q < n_seq; q++) P.seq_len[q] = (uint32_t)(h_off[q + 1] - h_off[q]);  // (a kept mate is not empty and shorter than 2^28)
    P.total = total;
    uint64_t qh[256], bh[256];
    for (int b = 0; b < 256; b++) {
        qh[b] = hist[b];
        bh[b] = hist[256 + b];
    }
    if ((rc = hc::plan_store(c, qh, bh, h_first.data(), n_kept, P))) return rc;
    cn.ms_plan = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    hc::release_store(c);
    N.raw_valid = false;
    if ((rc = hc::finish_store(c, P, N.next_bases.as<uint8_t>(), N.next_quals.as<uint8_t>(), N.next_off.as<uint64_t>(), N.next_first.as<uint32_t>(),
                               h_first.data(), n_kept)))
        return rc;
    // the new raw arrays become the kept ones
    N.bases.swap(N.next_bases);
    N.quals.swap(N.next_quals);
    N.off.swap(N.next_off);
    N.first.swap(N.next_first);
    N.h_off.swap(h_off);
    N.h_first.swap(h_first);
    N.total = total;
    N.raw_valid = true;
    N.prev_traded = true;  // the store this call read lies in the next_* blocks now
    N.prev_reads = n_reads_old;
    N.prev_seq = n_seq_old;
    N.prev_total = total_old;
    cn.ms_device += ms_b;
    return HC_OK;
}

extern "C" int hc_sr_set_next_reads(hc_ctx* c, const hc_sr_next_entry* entries, uint64_t n, const uint8_t* extra_seq, const uint8_t* extra_qual,
                                    uint64_t n_extra, const hc_sr_next_settings* settings, int32_t* new_id, uint32_t* status,
                                    hc_sr_next_counts* counts) {
    const char* me = "hc_sr_set_next_reads: ";
    if (!c || !settings || (n && (!entries || !new_id || !status)) || (n_extra && (!extra_seq || !extra_qual)))
        return fail(HC_ERR_ARG, std::string(me) + "null argument");
    if (n >= (1ull << 31)) return fail(HC_ERR_ARG, std::string(me) + "2^31 entries or more");
    hc_ctx::SrNext& N = c->srn;
    if (!N.keep) return fail(HC_ERR_STATE, std::string(me) + "hc_sr_keep_device is off");
    if (!c->have_reads || !N.raw_valid) return fail(HC_ERR_STATE, std::string(me) + "no store whose raw arrays were kept (hc_sr_keep_device, then hc_set_reads)");
    hc_sr_next_counts cn;
    memset(&cn, 0, sizeof cn);
    if (counts) *counts = cn;
    if (n == 0) {
        N.prev_traded = false;  // (hc_sr_fastq_write_text: the store this call read is the one in place)
        return HC_SR_NEXT_EMPTY;
    }
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint32_t n_reads_old = (uint32_t)(N.h_first.size() - 1);
    const hc::SrNextSources S{c->sr.kept_valid ? c->sr.kept_bytes : 0, n_extra, N.off.as<uint64_t>(), N.first.as<uint32_t>(), n_reads_old};
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n + 1, sizeof(uint64_t));
    int rc;
    if ((rc = N.entries.ensure(n * sizeof(hc_sr_next_entry))) || (rc = N.status.ensure(n * sizeof(uint32_t))) ||
        (rc = N.cnt.ensure((n + 1) * sizeof(uint64_t))) || (rc = N.bytes.ensure((n + 1) * sizeof(uint64_t))) ||
        (rc = N.cnt_off.ensure((n + 1) * sizeof(uint64_t))) || (rc = N.byte_off.ensure((n + 1) * sizeof(uint64_t))) ||
        (rc = N.temp.ensure(scan_bytes ? scan_bytes : 16)) || (rc = N.hist.ensure(512 * sizeof(unsigned long long))) ||
        (rc = N.extra_seq.ensure(n_extra ? n_extra : 1)) || (rc = N.extra_qual.ensure(n_extra ? n_extra : 1)))
        return rc;
    const hc::SrNextBytes B{{c->sr.seq.as<uint8_t>(), N.extra_seq.as<uint8_t>(), N.bases.as<uint8_t>()},
                            {c->sr.qual.as<uint8_t>(), N.extra_qual.as<uint8_t>(), N.quals.as<uint8_t>()}};
    HC_HIP(hipMemcpyAsync(N.entries.p, entries, n * sizeof(hc_sr_next_entry), hipMemcpyHostToDevice, s));
    if (n_extra) {
        HC_HIP(hipMemcpyAsync(N.extra_seq.p, extra_seq, n_extra, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(N.extra_qual.p, extra_qual, n_extra, hipMemcpyHostToDevice, s));
    }
    float ms_a = 0;
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_next_launch_check(N.entries.as<hc_sr_next_entry>(), n, S, B, settings->keep_singletons, N.status.as<uint32_t>(), N.cnt.as<uint64_t>(),
                                    N.bytes.as<uint64_t>(), s));
    HC_HIP(hc::prims::exclusive_sum(N.temp.p, N.temp.cap, N.cnt.as<uint64_t>(), N.cnt_off.as<uint64_t>(), n + 1, s));
    HC_HIP(hc::prims::exclusive_sum(N.temp.p, N.temp.cap, N.bytes.as<uint64_t>(), N.byte_off.as<uint64_t>(), n + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    uint64_t tot[2] = {0, 0};  // kept | sequences << 32, bytes
    HC_HIP(hipMemcpyAsync(&tot[0], N.cnt_off.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&tot[1], N.byte_off.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(status, N.status.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_a, c->ev0, c->ev1));
    const uint32_t n_kept = (uint32_t)tot[0], n_seq = (uint32_t)(tot[0] >> 32);
    const uint64_t total = tot[1];
    {
        int32_t rank = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t st = status[i];
            new_id[i] = st == HC_SR_NEXT_KEPT ? rank++ : -1;
            cn.n_kept += st == HC_SR_NEXT_KEPT;
            cn.n_dropped_empty += st == HC_SR_NEXT_DROPPED_EMPTY;
            cn.n_dropped_n_rate += st == HC_SR_NEXT_DROPPED_N_RATE;
            cn.n_dropped_short += st == HC_SR_NEXT_DROPPED_SHORT;
            cn.n_bad += st == HC_SR_NEXT_BAD_ENTRY;
        }
    }
    cn.n_seq = n_seq;
    cn.n_bytes = total;
    cn.ms_device = ms_a;
    if (counts) *counts = cn;
    if (cn.n_kept != n_kept) return fail(HC_ERR_STATE, std::string(me) + "the statuses and the device's count of survivors disagree");
    if (n_kept == 0) {  // the old store stays
        N.prev_traded = false;
        return HC_SR_NEXT_EMPTY;
    }
    if ((rc = hc::sr_next_store(c, n, n_extra, n_kept, n_seq, total, cn))) return rc;
    if (counts) *counts = cn;
    return HC_OK;
}

extern "C" int hc_sr_next_reads_fetch(hc_ctx* c, uint8_t* bases, uint8_t* quals, uint64_t cap_bytes, uint64_t* seq_off, uint32_t* read_first_seq,
                                      uint64_t cap_seq, uint64_t* n_bytes, uint64_t* n_seq, uint64_t* n_reads) {
    const char* me = "hc_sr_next_reads_fetch: ";
    if (!c || !n_bytes || !n_seq || !n_reads) return fail(HC_ERR_ARG, std::string(me) + "null argument");
    const hc_ctx::SrNext& N = c->srn;
    if (!N.keep || !N.raw_valid) return fail(HC_ERR_STATE, std::string(me) + "no kept raw arrays (hc_sr_keep_device, then hc_set_reads)");
    *n_bytes = N.total;
    *n_seq = N.h_off.size() - 1;
    *n_reads = N.h_first.size() - 1;
    if (!bases || !quals || !seq_off || !read_first_seq || cap_bytes < N.total || cap_seq < *n_seq)
        return fail(HC_ERR_ARG, std::string(me) + "a buffer is missing or too small (the counts hold the need)");
    HC_HIP(hipSetDevice(c->device));
    if (N.total) {
        HC_HIP(hipMemcpyAsync(bases, N.bases.p, N.total, hipMemcpyDeviceToHost, c->stream));
        HC_HIP(hipMemcpyAsync(quals, N.quals.p, N.total, hipMemcpyDeviceToHost, c->stream));
    }
    memcpy(seq_off, N.h_off.data(), N.h_off.size() * sizeof(uint64_t));
    memcpy(read_first_seq, N.h_first.data(), N.h_first.size() * sizeof(uint32_t));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}
