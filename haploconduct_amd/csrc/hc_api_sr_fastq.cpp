// hc_api_sr_fastq.cpp — hc_sr_fastq_write_text / hc_sr_fastq_text_fetch (include/hcsr.h): the bytes of singles.fastq, paired1.fastq,
// paired2.fastq and removed_tip_sequences.fastq (reference src/SRBuilder.cpp:1386-1556) from the raw arrays the context keeps.  Files 0 - 2
// are the current store's; the tips are reads of the store the last next-store call read, which hc_ctx::SrNext keeps track of.  The
// kernels of hc_sr_fastq_kernels.hip around one exclusive sum (hc_prims.hip): sizes, sum, boundaries, write — four launches whatever the
// sizes.  Everything is checked before the kept text is dropped: an error leaves it as it was.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr_fastq.h"

namespace {
int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }
}  // namespace

extern "C" {

int hc_sr_fastq_write_text(hc_ctx* c, const uint32_t* tips, uint64_t n_tips, const uint32_t* vertex_read, uint64_t n_vertices,
                           hc_sr_fastq_counts* counts) {
    const char* me = "hc_sr_fastq_write_text";
    if (!c || !counts || (n_tips && (!tips || !vertex_read))) return fail(me, HC_ERR_ARG, "null argument");
    memset(counts, 0, sizeof *counts);
    hc_ctx::SrNext& N = c->srn;
    hc_ctx::SrFastq& F = c->sr_fastq;
    if (!N.keep) return fail(me, HC_ERR_STATE, "hc_sr_keep_device is off");
    if (!c->have_reads || !N.raw_valid || N.h_first.empty())
        return fail(me, HC_ERR_STATE, "no store whose raw arrays were kept (hc_sr_keep_device, then hc_set_reads)");
    if (n_tips >= (1ull << 32)) return fail(me, HC_ERR_ARG, "2^32 tips or more");
    const uint32_t n_reads = (uint32_t)(N.h_first.size() - 1);
    const hc::fastq::Store cur{N.bases.as<uint8_t>(), N.quals.as<uint8_t>(), N.off.as<uint64_t>(), N.first.as<uint32_t>(), n_reads};
    // the store the last next-store call read: the traded blocks after a replacement, the current ones otherwise
    const hc::fastq::Store old = N.prev_traded ? hc::fastq::Store{N.next_bases.as<uint8_t>(), N.next_quals.as<uint8_t>(), N.next_off.as<uint64_t>(),
                                                                  N.next_first.as<uint32_t>(), N.prev_reads}
                                               : cur;
    std::vector<uint32_t> tip_reads(n_tips);
    for (uint64_t k = 0; k < n_tips; k++) {  // tips_vec.push_back(*read), :1302, :1309: the stored read of the tip's vertex
        if (tips[k] >= n_vertices) return fail(me, HC_ERR_ARG, "a tip vertex is not below n_vertices");
        const uint32_t r = vertex_read[tips[k]];
        if (r >= old.n_reads) return fail(me, HC_ERR_ARG, "vertex_read of a tip is no read of the store the last next-store call read");
        tip_reads[k] = r;
    }
    HC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t n_it = hc::fastq::n_items(n_reads, n_tips);
    int rc;
    if ((rc = F.sizes.ensure((n_it + 1) * 8)) || (rc = F.temp.ensure(hc::prims::scan_temp_bytes(n_it + 1, sizeof(uint64_t)))) ||
        (rc = F.counters.ensure(hc::fastq::kCounterWords * 8)) || (rc = F.tip_reads.ensure(n_tips ? n_tips * 4 : 16)))
        return rc;
    F.drop();
    if (n_tips) HC_HIP(hipMemcpyAsync(F.tip_reads.p, tip_reads.data(), n_tips * 4, hipMemcpyHostToDevice, s));
    const hc::fastq::Tips T{old, F.tip_reads.as<uint32_t>(), n_tips};
    uint64_t* d_sizes = F.sizes.as<uint64_t>();
    unsigned long long* d_counters = F.counters.as<unsigned long long>();
    float ms = 0;
    // sizes, their sum, the boundaries
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hipMemsetAsync(d_counters, 0, hc::fastq::kCounterWords * 8, s));
    HC_HIP(hc::fastq::launch_sizes(cur, T, d_sizes, d_counters, s));
    HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, d_sizes, d_sizes, n_it + 1, s));
    HC_HIP(hc::fastq::launch_bounds(n_reads, n_tips, d_sizes, d_counters, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    unsigned long long h[hc::fastq::kCounterWords];
    HC_HIP(hipMemcpyAsync(h, d_counters, sizeof h, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device = ms;
    const uint64_t total = h[8];
    if ((rc = F.text.ensure(total ? total : 1))) return rc;
    HC_HIP(hipEventRecord(c->ev0, s));
    if (total) HC_HIP(hc::fastq::launch_write(cur, T, d_sizes, F.text.as<char>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    counts->ms_device += ms;
    for (int f = 0; f < 4; f++) {
        counts->n_records[f] = h[f];
        counts->n_bytes[f] = h[5 + f] - h[4 + f];
    }
    for (int f = 0; f < 5; f++) F.bound[f] = h[4 + f];
    F.valid = true;
    return HC_OK;
}

int hc_sr_fastq_text_fetch(hc_ctx* c, uint32_t file, uint64_t first, uint64_t count, char* dst) {
    const char* me = "hc_sr_fastq_text_fetch";
    if (!c) return fail(me, HC_ERR_ARG, "null context");
    if (file > HC_SR_FASTQ_TIPS) return fail(me, HC_ERR_ARG, "no such file");
    const hc_ctx::SrFastq& F = c->sr_fastq;
    if (!F.valid) return fail(me, HC_ERR_STATE, "no text on the device (hc_sr_fastq_write_text first; replacing the raw arrays drops it)");
    const uint64_t n = F.bound[file + 1] - F.bound[file];
    if (first > n || count > n - first) return fail(me, HC_ERR_ARG, "range beyond the file");
    if (count == 0) return HC_OK;
    if (!dst) return fail(me, HC_ERR_ARG, "null destination");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(dst, F.text.as<char>() + F.bound[file] + first, count, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}

}  // extern "C"
