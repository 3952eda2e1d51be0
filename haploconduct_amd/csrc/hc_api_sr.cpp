// hc_api_sr.cpp — hc_sr_consensus (include/hcsr.h): SRBuilder::consensus / consensus_pos (reference src/SRBuilder.cpp:289-535) for a
// batch of layouts on the device.  The host builds what depends on libm — the per-quality log10 terms and the table of one- and
// two-member columns, once per read set and min_qual —, the kernels of hc_sr_kernels.hip do the rest, and the columns they could not
// decide by comparisons come back as four sums that host threads finish with the reference's expressions (host/SrConsensus.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr.h"
#include "host/SrConsensus.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {

int build_tables(hc_ctx* c, double min_qual) {
    if (c->sr.tables_valid && memcmp(&c->sr.table_min_qual, &min_qual, sizeof(double)) == 0) return HC_OK;
    c->sr.tables_valid = false;
    std::vector<double> terms(2 * hc::kSrQIdx, 0.0);
    std::vector<uint32_t> qs;
    for (uint32_t i = 0; i < hc::kSrQIdx; i++) {
        if (c->sr_qbyte[i] == 255) continue;
        hc::sr::terms((int)c->sr_qbyte[i], terms[i], terms[hc::kSrQIdx + i]);
        qs.push_back(c->sr_qbyte[i]);
    }
    std::vector<uint8_t> table(HC_SR_TABLE_BYTES);
    hc::sr::build_table(min_qual, qs, table.data());
    int rc = c->sr.terms.ensure(terms.size() * sizeof(double));
    if (rc == HC_OK) rc = c->sr.qbyte.ensure(hc::kSrQIdx);
    if (rc == HC_OK) rc = c->sr.table.ensure(table.size());
    if (rc) return rc;
    HC_HIP(hipMemcpyAsync(c->sr.terms.p, terms.data(), terms.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipMemcpyAsync(c->sr.qbyte.p, c->sr_qbyte, hc::kSrQIdx, hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipMemcpyAsync(c->sr.table.p, table.data(), table.size(), hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));  // (the host vectors go out of scope)
    c->sr.tables_valid = true;
    c->sr.table_min_qual = min_qual;
    return HC_OK;
}

}  // namespace

extern "C" int hc_sr_consensus(hc_ctx* c, const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members, uint64_t n_members,
                               const hc_sr_settings* settings, int32_t* ret, uint32_t* status, uint64_t* out_off, uint8_t* cons_seq,
                               uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats) {
    if (!c || !settings || !out_off || !n_bytes || (n_layouts && (!layouts || !ret || !status)) || (n_members && !members))
        return fail(HC_ERR_ARG, "hc_sr_consensus: null argument");
    if (!c->have_reads) return fail(HC_ERR_STATE, "hc_sr_consensus: hc_set_reads first");
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, "hc_sr_consensus: min_qual is NaN");
    if (n_layouts >= (1ull << 32) - 1 || n_members >= (1ull << 32)) return fail(HC_ERR_ARG, "hc_sr_consensus: more than 2^32 - 2 layouts or members");
    if (stats) memset(stats, 0, sizeof *stats);
    *n_bytes = 0;
    out_off[0] = 0;
    if (n_layouts == 0) return HC_OK;
    HC_HIP(hipSetDevice(c->device));
    int rc = build_tables(c, settings->min_qual);
    if (rc) return rc;
    hc_ctx::Sr& S = c->sr;
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n_layouts + 1, sizeof(uint64_t));
    if ((rc = S.layouts.ensure(n_layouts * sizeof(hc_sr_layout))) || (rc = S.members.ensure((n_members ? n_members : 1) * sizeof(hc_sr_member))) ||
        (rc = S.mem.ensure((n_members ? n_members : 1) * sizeof(hc::SrMember))) || (rc = S.info.ensure(n_layouts * sizeof(hc::SrLayoutInfo))) ||
        (rc = S.len.ensure((n_layouts + 1) * sizeof(uint64_t))) || (rc = S.off.ensure((n_layouts + 1) * sizeof(uint64_t))) ||
        (rc = S.temp.ensure(scan_bytes ? scan_bytes : 16)) || (rc = S.late.ensure(n_layouts * sizeof(uint32_t))) ||
        (rc = S.counter.ensure(sizeof(unsigned long long))))
        return rc;
    hipStream_t s = c->stream;
    float ms_a = 0, ms_b = 0;
    HC_HIP(hipMemcpyAsync(S.layouts.p, layouts, n_layouts * sizeof(hc_sr_layout), hipMemcpyHostToDevice, s));
    if (n_members) HC_HIP(hipMemcpyAsync(S.members.p, members, n_members * sizeof(hc_sr_member), hipMemcpyHostToDevice, s));
    const uint32_t minimum_support = settings->subreads_needed ? 2u : settings->min_clique_size;  // :421-427
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_launch_layouts(c->view, S.layouts.as<hc_sr_layout>(), n_layouts, S.members.as<hc_sr_member>(), n_members, minimum_support,
                                 settings->error_correction ? 1u : 0u, S.mem.as<hc::SrMember>(), S.info.as<hc::SrLayoutInfo>(), S.len.as<uint64_t>(), s));
    HC_HIP(hc::prims::exclusive_sum(S.temp.p, S.temp.cap, S.len.as<uint64_t>(), S.off.as<uint64_t>(), n_layouts + 1, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    std::vector<hc::SrLayoutInfo> info(n_layouts);
    HC_HIP(hipMemcpyAsync(info.data(), S.info.p, n_layouts * sizeof(hc::SrLayoutInfo), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(out_off, S.off.p, (n_layouts + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_a, c->ev0, c->ev1));
    for (uint64_t l = 0; l < n_layouts; l++) {
        ret[l] = info[l].ret;
        status[l] = info[l].status;
    }
    const uint64_t total = out_off[n_layouts];
    *n_bytes = total;
    if (stats) {
        stats->n_columns = total;
        stats->ms_device = ms_a;
    }
    if (total > cap || (total && (!cons_seq || !cons_qual)))
        return fail(HC_ERR_ARG, "hc_sr_consensus: cons_seq / cons_qual have no room (*n_bytes says how much is needed)");
    if (total == 0) return HC_OK;
    if ((rc = S.seq.ensure(total)) || (rc = S.qual.ensure(total))) return rc;
    // columns for the host: room for an eighth of all columns at first; the count tells when that was too little, and the kernel runs again
    uint64_t host_cap = std::max<uint64_t>(1u << 16, total / 8);
    unsigned long long n_host = 0;
    std::vector<uint32_t> late(n_layouts);
    for (int pass = 0; pass < 2; pass++) {
        if ((rc = S.host_cols.ensure(host_cap * sizeof(hc::SrHostColumn)))) return rc;
        HC_HIP(hipMemsetAsync(S.late.p, 0, n_layouts * sizeof(uint32_t), s));
        HC_HIP(hipMemsetAsync(S.counter.p, 0, sizeof(unsigned long long), s));
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::sr_launch_columns(c->view, c->n_cu, S.layouts.as<hc_sr_layout>(), n_layouts, S.mem.as<hc::SrMember>(), S.info.as<hc::SrLayoutInfo>(),
                                     S.off.as<uint64_t>(), S.terms.as<double>(), S.qbyte.as<uint8_t>(), S.table.as<uint8_t>(),
                                     hc::sr::safe_region_allowed(settings->min_qual) ? 1u : 0u, S.seq.as<uint8_t>(), S.qual.as<uint8_t>(),
                                     S.late.as<uint32_t>(), S.host_cols.as<hc::SrHostColumn>(), host_cap, S.counter.as<unsigned long long>(), s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(&n_host, S.counter.p, sizeof n_host, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        float ms = 0;
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_b += ms;
        if (n_host <= host_cap) break;
        if (pass == 1) return fail(HC_ERR_STATE, "hc_sr_consensus: the host's column count grew between two identical launches");
        host_cap = n_host;
    }
    std::vector<hc::SrHostColumn> cols(n_host);
    HC_HIP(hipMemcpyAsync(cons_seq, S.seq.p, total, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(cons_qual, S.qual.p, total, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(late.data(), S.late.p, n_layouts * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (n_host) HC_HIP(hipMemcpyAsync(cols.data(), S.host_cols.p, n_host * sizeof(hc::SrHostColumn), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    // the host's share: :348-396 with the host libm on the device's sums, spliced into the packed buffers
    const auto t0 = std::chrono::steady_clock::now();
    if (n_host) {
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)settings->n_threads, 64, n_host / 4096 + 1}));
        std::atomic<uint64_t> turn{0};
        const uint64_t block = 4096;
        const double min_qual = settings->min_qual;
        auto work = [&]() {
            for (uint64_t a = turn.fetch_add(block); a < n_host; a = turn.fetch_add(block)) {
                for (uint64_t i = a; i < std::min<uint64_t>(n_host, a + block); i++) {
                    const hc::SrHostColumn& h = cols[i];
                    uint8_t o[2];
                    if (hc::sr::finish(h.s[0], h.s[1], h.s[2], h.s[3], h.n, min_qual, o)) {
                        cons_seq[h.out] = o[0];
                        cons_qual[h.out] = o[1];
                    } else {
                        // (several threads may store the same value)
                        reinterpret_cast<std::atomic<uint32_t>*>(&late[h.layout])->fetch_or(hc::kSrLateNaN, std::memory_order_relaxed);
                    }
                }
            }
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; t++) th.emplace_back(work);
        work();
        for (auto& x : th) x.join();
    }
    // layouts that failed late (:528-532, an invalid symbol): their bytes leave the packed buffers
    bool any_late = false;
    for (uint64_t l = 0; l < n_layouts && !any_late; l++) any_late = late[l] != 0;
    if (any_late) {
        uint64_t w = 0;
        for (uint64_t l = 0; l < n_layouts; l++) {
            const uint64_t a = out_off[l], len = info[l].len;
            out_off[l] = w;
            if (late[l]) {
                status[l] = (late[l] & hc::kSrLateBadSymbol) ? HC_SR_BAD_SYMBOL : HC_SR_NAN;
                if (late[l] & hc::kSrLateBadSymbol) ret[l] = 0;
                continue;
            }
            if (len && w != a) {
                memmove(cons_seq + w, cons_seq + a, len);
                memmove(cons_qual + w, cons_qual + a, len);
            }
            w += len;
        }
        out_off[n_layouts] = w;
        *n_bytes = w;
    }
    if (stats) {
        stats->n_columns = *n_bytes;
        stats->n_host_columns = n_host;
        stats->ms_device = (double)ms_a + ms_b;
        stats->ms_host_finish = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return HC_OK;
}
