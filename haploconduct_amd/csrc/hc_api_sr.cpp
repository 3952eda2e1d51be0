// hc_api_sr.cpp — hc_sr_consensus (include/hcsr.h): SRBuilder::consensus / consensus_pos (reference src/SRBuilder.cpp:289-535) for a
// batch of layouts on the device.  The host builds what depends on libm — the per-quality log10 terms and the table of one- and
// two-member columns, once per read set and min_qual —, the kernels of hc_sr_kernels.hip do the rest, and the columns they could not
// decide by comparisons come back as four sums that host threads finish with the reference's expressions (host/SrConsensus.h).
// hc_sr_consensus is in parts (hc_ctx.h: sr_consensus_begin / _room / _run) so that hc_sr_edge_merge (hc_api_sr_edge.cpp), whose layouts are
// on the device already, runs the same code from there on.
// hc_sr_merge_self_overlaps and hc_sr_merge_self_overlaps_kept: SRBuilder::merge_self_overlap (:872-955) for a batch of pairs, at the end
// of this file, with hc_sr_kept_load / hc_sr_kept_fetch.  All calls build their consensus tables with sr_tables and run their host loops
// with in_blocks (host/InBlocks.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hcsr.h"
#include "hc_ctx.h"
#include "hc_prims.h"
#include "hc_sr.h"
#include "hc_sr_merge_next.h"
#include "hc_sr_next.h"
#include "hc_sr_self.h"
#include "host/EnvKnobs.h"
#include "host/InBlocks.h"
#include "host/SrConsensus.h"
#include "host/SrSelfOverlap.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {

// The consensus tables (host/SrConsensus.h) for the quality values q_of[i] = byte - 33 of term index i (255: none) and min_qual, on the
// device: built and uploaded unless T holds them already.  The consensus call's term index is the store's quality index, the merge
// call's the quality value itself.
int sr_tables(hc_ctx* c, hc_ctx::SrTables& T, const uint8_t* q_of, double min_qual) {
    constexpr uint32_t kQDim = hc::sr::kQDim;
    static_assert(sizeof T.q_of == kQDim, "one entry per term index");
    if (T.valid && memcmp(&T.min_qual, &min_qual, sizeof(double)) == 0 && memcmp(T.q_of, q_of, kQDim) == 0) return HC_OK;
    T.valid = false;
    std::vector<double> terms(2 * kQDim, 0.0);
    std::vector<uint32_t> qs;
    for (uint32_t i = 0; i < kQDim; i++) {
        if (q_of[i] == 255) continue;
        hc::sr::terms((int)q_of[i], terms[i], terms[kQDim + i]);
        qs.push_back(q_of[i]);
    }
    std::vector<uint8_t> table(HC_SR_TABLE_BYTES);
    hc::sr::build_table(min_qual, qs, table.data());
    int rc;
    if ((rc = T.terms.ensure(terms.size() * sizeof(double))) || (rc = T.qbyte.ensure(kQDim)) || (rc = T.table.ensure(table.size()))) return rc;
    HC_HIP(hipMemcpyAsync(T.terms.p, terms.data(), terms.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipMemcpyAsync(T.qbyte.p, q_of, kQDim, hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipMemcpyAsync(T.table.p, table.data(), table.size(), hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));  // (the host vectors go out of scope)
    T.valid = true;
    T.has_nan = memchr(table.data(), hc::sr::kEntryNaN, table.size()) != nullptr;
    T.min_qual = min_qual;
    memcpy(T.q_of, q_of, kQDim);
    return HC_OK;
}

}  // namespace

int hc::sr_consensus_begin(hc_ctx* c, uint64_t* out_off, uint64_t* n_bytes, hc_sr_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    *n_bytes = 0;
    out_off[0] = 0;
    c->sr.kept_valid = false;
    c->sr.kept_bytes = 0;
    return HC_OK;
}

int hc::sr_consensus_room(hc_ctx* c, const hc_sr_settings* settings, uint64_t n_layouts, uint64_t n_members) {
    hc_ctx::Sr& S = c->sr;
    HC_HIP(hipSetDevice(c->device));
    int rc = sr_tables(c, S.tables, c->sr_qbyte, settings->min_qual);
    if (rc) return rc;
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n_layouts + 1, sizeof(uint64_t));
    if ((rc = S.layouts.ensure(n_layouts * sizeof(hc_sr_layout))) || (rc = S.members.ensure((n_members ? n_members : 1) * sizeof(hc_sr_member))) ||
        (rc = S.mem.ensure((n_members ? n_members : 1) * sizeof(hc::SrMember))) || (rc = S.info.ensure(n_layouts * sizeof(hc::SrLayoutInfo))) ||
        (rc = S.len.ensure((n_layouts + 1) * sizeof(uint64_t))) || (rc = S.off.ensure((n_layouts + 1) * sizeof(uint64_t))) ||
        (rc = S.temp.ensure(scan_bytes ? scan_bytes : 16)) || (rc = S.late.ensure(n_layouts * sizeof(uint32_t))) ||
        (rc = S.counter.ensure(sizeof(unsigned long long))))
        return rc;
    return HC_OK;
}

extern "C" int hc_sr_consensus(hc_ctx* c, const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members, uint64_t n_members,
                               const hc_sr_settings* settings, int32_t* ret, uint32_t* status, uint64_t* out_off, uint8_t* cons_seq,
                               uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats) {
    if (!c || !settings || !out_off || !n_bytes || (n_layouts && (!layouts || !ret || !status)) || (n_members && !members))
        return fail(HC_ERR_ARG, "hc_sr_consensus: null argument");
    if (!c->have_reads) return fail(HC_ERR_STATE, "hc_sr_consensus: hc_set_reads first");
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, "hc_sr_consensus: min_qual is NaN");
    if (n_layouts >= (1ull << 32) - 1 || n_members >= (1ull << 32)) return fail(HC_ERR_ARG, "hc_sr_consensus: more than 2^32 - 2 layouts or members");
    hc::sr_consensus_begin(c, out_off, n_bytes, stats);
    if (n_layouts) {
        int rc = hc::sr_consensus_room(c, settings, n_layouts, n_members);
        if (rc) return rc;
        hc_ctx::Sr& S = c->sr;
        HC_HIP(hipMemcpyAsync(S.layouts.p, layouts, n_layouts * sizeof(hc_sr_layout), hipMemcpyHostToDevice, c->stream));
        if (n_members) HC_HIP(hipMemcpyAsync(S.members.p, members, n_members * sizeof(hc_sr_member), hipMemcpyHostToDevice, c->stream));
    }
    return hc::sr_consensus_run(c, "hc_sr_consensus", n_layouts, n_members, settings, ret, status, out_off, cons_seq, cons_qual, cap, n_bytes, stats,
                                nullptr);
}

// From the layouts and members on the device (S.layouts, S.members; the blocks of sr_consensus_room) on.
int hc::sr_consensus_run(hc_ctx* c, const char* me, uint64_t n_layouts, uint64_t n_members, const hc_sr_settings* settings, int32_t* ret,
                         uint32_t* status, uint64_t* out_off, uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes,
                         hc_sr_stats* stats, bool* ret_late) {
    hc_ctx::Sr& S = c->sr;
    const bool keep = c->srn.keep;  // hc_sr_keep_device: the bytes stay on the device in their final form
    if (ret_late) *ret_late = false;
    if (n_layouts == 0) {
        S.kept_valid = keep;
        return HC_OK;
    }
    int rc;
    hipStream_t s = c->stream;
    float ms_a = 0, ms_b = 0;
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
    if ((rc = hc::sr::check_room(me, "cons_seq / cons_qual", "n_bytes", total, cap, cons_seq, cons_qual))) return rc;
    if (total == 0) {
        S.kept_valid = keep;
        return HC_OK;
    }
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
                                     S.off.as<uint64_t>(), S.tables.terms.as<double>(), S.tables.qbyte.as<uint8_t>(), S.tables.table.as<uint8_t>(),
                                     hc::sr::safe_region_allowed(settings->min_qual) ? 1u : 0u, S.seq.as<uint8_t>(), S.qual.as<uint8_t>(),
                                     S.late.as<uint32_t>(), S.host_cols.as<hc::SrHostColumn>(), host_cap, S.counter.as<unsigned long long>(), s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(&n_host, S.counter.p, sizeof n_host, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        float ms = 0;
        HC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_b += ms;
        if (n_host <= host_cap) break;
        if (pass == 1) return fail(HC_ERR_STATE, std::string(me) + ": the host's column count grew between two identical launches");
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
    std::vector<hc::SrPatch> patches(keep ? n_host : 0);
    hc::in_blocks(n_host, 4096, settings->n_threads, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            const hc::SrHostColumn& h = cols[i];
            uint8_t o[2];
            if (keep) patches[i] = hc::SrPatch{~0ull, 0, 0, {0, 0, 0, 0, 0, 0}};
            if (hc::sr::finish(h.s[0], h.s[1], h.s[2], h.s[3], h.n, settings->min_qual, o)) {
                cons_seq[h.out] = o[0];
                cons_qual[h.out] = o[1];
                if (keep) patches[i] = hc::SrPatch{h.out, o[0], o[1], {0, 0, 0, 0, 0, 0}};
            } else {
                // (several threads may store the same value)
                reinterpret_cast<std::atomic<uint32_t>*>(&late[h.layout])->fetch_or(hc::kSrLateNaN, std::memory_order_relaxed);
            }
        }
    });
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
                if (late[l] & hc::kSrLateBadSymbol) {
                    ret[l] = 0;
                    if (ret_late) *ret_late = true;
                }
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
    if (keep) {
        if (any_late) {  // (next to never: layouts left the packed buffers, and the kept bytes follow the host's)
            if (*n_bytes) {
                HC_HIP(hipMemcpyAsync(S.seq.p, cons_seq, *n_bytes, hipMemcpyHostToDevice, s));
                HC_HIP(hipMemcpyAsync(S.qual.p, cons_qual, *n_bytes, hipMemcpyHostToDevice, s));
            }
        } else if (n_host) {  // one scatter of the columns the host threads finished
            if ((rc = S.patches.ensure(n_host * sizeof(hc::SrPatch)))) return rc;
            HC_HIP(hipMemcpyAsync(S.patches.p, patches.data(), n_host * sizeof(hc::SrPatch), hipMemcpyHostToDevice, s));
            HC_HIP(hc::sr_launch_patch(S.patches.as<hc::SrPatch>(), n_host, total, S.seq.as<uint8_t>(), S.qual.as<uint8_t>(), s));
        }
        HC_HIP(hipStreamSynchronize(s));  // (the host vectors go out of scope)
        S.kept_bytes = *n_bytes;
        S.kept_valid = true;
    }
    if (stats) {
        stats->n_columns = *n_bytes;
        stats->n_host_columns = n_host;
        stats->ms_device = (double)ms_a + ms_b;
        stats->ms_host_finish = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return HC_OK;
}

// --------------------------------------------------------------------------------------------------------------------------------------
// hc_sr_merge_self_overlaps / hc_sr_merge_self_overlaps_kept: the pairs are checked and the batch's quality values collected — by host
// threads on the caller's arrays, or by sr_self_check_kernel on the bytes the context keeps —, the host builds what depends on libm (the
// log p table of the batch's quality values, by the scoring path's own builder; 1.0 / n; the consensus table), the scan kernel finds every
// pair's offset, the host decides the offsets inside the guard band (host/SrSelfOverlap.h), the merge kernel writes the merged reads at the
// offsets of an exclusive sum.  From the check on the two calls run the same functions (self_scan, self_host_pairs, self_merge): what
// differs is where the mates lie and where the merged reads go.
namespace {

struct SelfBatch {  // what the check leaves of a batch, over its valid pairs
    std::vector<uint32_t> skip;  // the pairs' statuses before the scan: 0 = scanned
    uint8_t qs_seen[96] = {0};   // the quality values byte - 33 that occur
    uint32_t max_len = 0, max_first = 0;
    uint64_t n_offsets = 0, n_valid = 0;
};

struct SelfWork {  // what the scan and the host's share leave for the merge
    std::vector<uint64_t> len;  // n_pairs + 1: the merged reads' lengths, the last 0
    std::vector<int32_t> mpos;  // the offset of a pair the merge kernel writes, -1: not the device's columns
    // pairs the host finishes: (pair, the offset its scan goes on from)
    std::vector<std::pair<uint64_t, uint32_t>> host_pairs;
    struct Out {
        std::vector<uint8_t> seq, qual;
    };
    std::vector<Out> host_out;  // their merged reads
    float ms_scan = 0, ms_merge = 0;
    double ms_host = 0;
};

void self_begin(const SelfBatch& B, uint64_t n_pairs, int32_t* overlap_pos, double* score, uint32_t* status, SelfWork& W) {
    W.len.assign(n_pairs + 1, 0);
    W.mpos.assign(n_pairs, -1);
    for (uint64_t i = 0; i < n_pairs; i++) {
        overlap_pos[i] = -1;
        score[i] = 0;
        status[i] = B.skip[i];
    }
}

// The tables, the scan of the pairs on the device (S.pairs, S.skip) over d_seq / d_qual, and the scan's verdicts: a pair the device
// decided gets its outputs, the others join W.host_pairs.  Runs only for a batch with an offset to try.
int self_scan(hc_ctx* c, const std::string& me, const SelfBatch& B, const uint8_t* d_seq, const uint8_t* d_qual, const hc_sr_pair* pairs,
              uint64_t n_pairs, const hc_sr_self_settings* settings, int32_t* overlap_pos, double* score, uint32_t* status, SelfWork& W) {
    hc_ctx::SrSelf& S = c->sr_self;
    hipStream_t s = c->stream;
    int rc;
    const auto t0 = std::chrono::steady_clock::now();
    // tables: log p by the scoring path's builder for the batch's values (row = rank of the value), 1.0 / n, the consensus table
    std::vector<int> phred;
    uint8_t qmap[256], q_of[hc::sr::kQDim];
    memset(qmap, 0, sizeof qmap);
    memset(q_of, 255, sizeof q_of);
    for (uint32_t q = 0; q < hc::srself::kQ; q++) {
        if (!B.qs_seen[q]) continue;
        qmap[q + 33] = (uint8_t)phred.size();
        phred.push_back((int)q);
        q_of[q] = (uint8_t)q;
    }
    std::vector<double> lut;
    if (!hc::build_log_table_u16(phred, c->settings.mismatch, lut)) return fail(HC_ERR_STATE, me + "the log table is not symmetric");
    std::vector<double> inv_n((size_t)B.max_len + 1, 0.0);
    for (uint32_t k = 1; k <= B.max_len; k++) inv_n[k] = 1.0 / (double)k;  // :137
    if ((rc = sr_tables(c, S.tables, q_of, settings->min_qual))) return rc;
    hc::SrSelfParams prm;
    int log2_width = -49;
    {  // test knob: a wider guard band, so that the host-decided path runs
        const int v = hc::env::i(hc::env::Knob::SR_SELF_BAND_LOG2, log2_width);
        if (v >= -60 && v <= -2) log2_width = v;
    }
    prm.band = hc::threshold_band(settings->min_score, log2_width);
    prm.always = settings->min_score < 0 ? 1u : 0u;
    prm.min_overlap = settings->min_overlap;
    prm.min_read_len = c->settings.min_read_len;
    prm.K = (uint32_t)phred.size();
    prm.lut_doubles = (uint32_t)lut.size();
    prm.inv_len = (uint32_t)inv_n.size();
    if ((rc = S.qmap.ensure(256)) || (rc = S.lut.ensure(lut.size() * sizeof(double))) || (rc = S.inv_n.ensure(inv_n.size() * sizeof(double))) ||
        (rc = S.res.ensure(n_pairs * sizeof(hc::SrSelfScan))))
        return rc;
    W.ms_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HC_HIP(hipMemcpyAsync(S.qmap.p, qmap, 256, hipMemcpyHostToDevice, s));
    HC_HIP(hipMemcpyAsync(S.lut.p, lut.data(), lut.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HC_HIP(hipMemcpyAsync(S.inv_n.p, inv_n.data(), inv_n.size() * sizeof(double), hipMemcpyHostToDevice, s));
    const uint32_t lanes = 64u * std::max(1u, std::min(hc::kSelfMaxChunk / 64u, (B.max_first + 63u) / 64u));
    std::vector<hc::SrSelfScan> res(n_pairs);
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_self_launch_scan(c->n_cu, lanes, d_seq, d_qual, S.pairs.as<hc_sr_pair>(), S.skip.as<uint32_t>(), n_pairs, S.qmap.as<uint8_t>(),
                                   S.lut.as<double>(), S.inv_n.as<double>(), prm, S.res.as<hc::SrSelfScan>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipMemcpyAsync(res.data(), S.res.p, n_pairs * sizeof(hc::SrSelfScan), hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&W.ms_scan, c->ev0, c->ev1));
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (B.skip[i] || res[i].p < 0) continue;
        if (res[i].kind == hc::kSelfHit && !S.tables.has_nan) {
            overlap_pos[i] = res[i].p;
            score[i] = exp(res[i].x);  // :138
            status[i] = HC_SR_SELF_MERGED;
            W.len[i] = (uint64_t)pairs[i].len2 + (uint32_t)res[i].p;  // :890
            W.mpos[i] = res[i].p;
        } else {
            W.host_pairs.emplace_back(i, (uint32_t)res[i].p);
        }
    }
    return HC_OK;
}

// The host's share: the scan of W.host_pairs[k] goes on from the offset in the band with the host's libm, as the mirror walks it, on
// the mates M[k] in host memory.
void self_host_pairs(hc_ctx* c, const hc_sr_self_settings* settings, const std::vector<hc::srself::Mates>& M, int32_t* overlap_pos, double* score,
                     uint32_t* status, SelfWork& W) {
    W.host_out.resize(W.host_pairs.size());
    if (W.host_pairs.empty()) return;
    const auto t0 = std::chrono::steady_clock::now();
    const hc::srself::Tables T(c->settings.mismatch, c->settings.min_read_len);
    hc::in_blocks(W.host_pairs.size(), 1, std::max(1u, settings->n_threads), [&](uint64_t a, uint64_t b) {
        for (uint64_t k = a; k < b; k++) {
            const uint64_t i = W.host_pairs[k].first;
            overlap_pos[i] = hc::srself::scan_pair(T, M[k], W.host_pairs[k].second, *settings, &score[i], W.host_out[k].seq, W.host_out[k].qual);
            if (overlap_pos[i] < 0) continue;
            status[i] = HC_SR_SELF_MERGED;
            W.len[i] = W.host_out[k].seq.size();
        }
    });
    W.ms_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// out_off[i] = base + the bytes of the pairs before i; returns the bytes of all
uint64_t self_offsets(const SelfWork& W, uint64_t n_pairs, uint64_t base, const uint32_t* status, uint64_t* out_off, hc_sr_self_stats* stats,
                      uint64_t n_offsets) {
    uint64_t total = 0, n_merged = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        out_off[i] = base + total;
        total += W.len[i];
        n_merged += status[i] == HC_SR_SELF_MERGED;
    }
    out_off[n_pairs] = base + total;
    if (stats) {
        stats->n_merged = n_merged;
        stats->n_host_pairs = W.host_pairs.size();
        stats->n_offsets = n_offsets;
        stats->ms_device = W.ms_scan;
        stats->ms_host = W.ms_host;
    }
    return total;
}

// The merged reads of the pairs the device decided: offsets by an exclusive sum on the device, one lane per column, into d_out_seq /
// d_out_qual (room for `total` bytes).  Enqueues and records the events; the caller waits and reads W.ms_merge with self_merge_ms.
int self_merge(hc_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, uint64_t n_pairs, const SelfWork& W, uint64_t total, uint8_t* d_out_seq,
               uint8_t* d_out_qual) {
    hc_ctx::SrSelf& S = c->sr_self;
    hipStream_t s = c->stream;
    const size_t scan_bytes = hc::prims::scan_temp_bytes(n_pairs + 1, sizeof(uint64_t));
    int rc;
    if ((rc = S.len.ensure((n_pairs + 1) * sizeof(uint64_t))) || (rc = S.off.ensure((n_pairs + 1) * sizeof(uint64_t))) ||
        (rc = S.mpos.ensure(n_pairs * sizeof(int32_t))) || (rc = S.temp.ensure(scan_bytes ? scan_bytes : 16)))
        return rc;
    HC_HIP(hipMemcpyAsync(S.len.p, W.len.data(), (n_pairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HC_HIP(hipMemcpyAsync(S.mpos.p, W.mpos.data(), n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::prims::exclusive_sum(S.temp.p, S.temp.cap, S.len.as<uint64_t>(), S.off.as<uint64_t>(), n_pairs + 1, s));
    HC_HIP(hc::sr_self_launch_merge(d_seq, d_qual, S.pairs.as<hc_sr_pair>(), n_pairs, S.mpos.as<int32_t>(), S.off.as<uint64_t>(), total,
                                    S.tables.terms.as<double>(), S.tables.table.as<uint8_t>(), d_out_seq, d_out_qual, s));
    HC_HIP(hipEventRecord(c->ev1, s));
    return HC_OK;
}

int self_merge_ms(hc_ctx* c, SelfWork& W, hc_sr_self_stats* stats) {
    HC_HIP(hipEventElapsedTime(&W.ms_merge, c->ev0, c->ev1));
    if (stats) stats->ms_device = (double)W.ms_scan + W.ms_merge;
    return HC_OK;
}

// The kept consensus bytes get room for `bytes` and the check kernel's padding behind them, their contents preserved.  (The headroom of
// an eighth, as hc_scratch::ensure's, is less than the padding for a small block.)
int kept_reserve(hc_ctx* c, uint64_t bytes) {
    hc_ctx::Sr& K = c->sr;
    const size_t want = bytes + hc::kSelfPad;
    for (hc_scratch* b : {&K.seq, &K.qual})
        if (b->cap < want)
            if (const int rc = b->grow_keep(want + want / 8, K.kept_bytes, c->stream)) return rc;
    return HC_OK;
}

}  // namespace

extern "C" int hc_sr_merge_self_overlaps(hc_ctx* c, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes, const hc_sr_pair* pairs,
                                         uint64_t n_pairs, const hc_sr_self_settings* settings, int32_t* overlap_pos, double* score,
                                         uint32_t* status, uint64_t* out_off, uint8_t* merged_seq, uint8_t* merged_qual, uint64_t cap,
                                         uint64_t* n_out, hc_sr_self_stats* stats) {
    const std::string me = "hc_sr_merge_self_overlaps: ";
    if (!c || !settings || !out_off || !n_out || (n_pairs && (!pairs || !overlap_pos || !score || !status)) || (n_bytes && (!seq || !qual)))
        return fail(HC_ERR_ARG, me + "null argument");
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, me + "min_qual is NaN");
    if (n_pairs >= (1ull << 32) - 1) return fail(HC_ERR_ARG, me + "more than 2^32 - 2 pairs");
    if (stats) memset(stats, 0, sizeof *stats);
    *n_out = 0;
    out_off[0] = 0;
    if (n_pairs == 0) return HC_OK;
    HC_HIP(hipSetDevice(c->device));
    const auto t_host0 = std::chrono::steady_clock::now();
    const unsigned n_thr = std::max(1u, settings->n_threads);
    // the pairs' checks and the quality values of the batch
    SelfBatch B;
    B.skip.resize(n_pairs);
    const uint64_t check_block = 1024, n_check_blocks = (n_pairs + check_block - 1) / check_block;
    std::vector<std::array<uint8_t, 128>> seen(n_check_blocks);
    std::vector<uint32_t> block_max(n_check_blocks, 0);
    hc::in_blocks(n_pairs, check_block, n_thr, [&](uint64_t a, uint64_t b) {
        std::array<uint8_t, 128>& sn = seen[a / check_block];
        sn.fill(0);
        uint32_t mx = 0;
        for (uint64_t i = a; i < b; i++) {
            B.skip[i] = hc::srself::check_pair(seq, qual, n_bytes, pairs[i]);
            if (B.skip[i]) continue;
            const hc_sr_pair& P = pairs[i];
            for (uint32_t k = 0; k < P.len1; k++) sn[qual[P.off1 + k] & 127u] = 1;
            for (uint32_t k = 0; k < P.len2; k++) sn[qual[P.off2 + k] & 127u] = 1;
            mx = std::max({mx, P.len1, P.len2});
        }
        block_max[a / check_block] = mx;
    });
    for (uint64_t b = 0; b < n_check_blocks; b++) {
        B.max_len = std::max(B.max_len, block_max[b]);
        for (uint32_t q = 33; q <= 126; q++) B.qs_seen[q - 33] |= seen[b][q];
    }
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (B.skip[i]) continue;
        B.n_valid++;
        const uint32_t f = hc::srself::first_offset(pairs[i].len1, settings->min_overlap);
        B.n_offsets += f;
        B.max_first = std::max(B.max_first, f);
    }
    if (stats) stats->n_offsets = B.n_offsets;
    hc_ctx::SrSelf& S = c->sr_self;
    hipStream_t s = c->stream;
    SelfWork W;
    self_begin(B, n_pairs, overlap_pos, score, status, W);
    W.ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    int rc = HC_OK;
    if (B.n_valid && B.max_first) {
        if ((rc = S.seq.ensure(n_bytes)) || (rc = S.qual.ensure(n_bytes)) || (rc = S.pairs.ensure(n_pairs * sizeof(hc_sr_pair))) ||
            (rc = S.skip.ensure(n_pairs * sizeof(uint32_t))))
            return rc;
        HC_HIP(hipMemcpyAsync(S.seq.p, seq, n_bytes, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.qual.p, qual, n_bytes, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.pairs.p, pairs, n_pairs * sizeof(hc_sr_pair), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.skip.p, B.skip.data(), n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if ((rc = self_scan(c, me, B, S.seq.as<uint8_t>(), S.qual.as<uint8_t>(), pairs, n_pairs, settings, overlap_pos, score, status, W))) return rc;
    }
    std::vector<hc::srself::Mates> mates(W.host_pairs.size());
    for (size_t k = 0; k < mates.size(); k++) {
        const hc_sr_pair& P = pairs[W.host_pairs[k].first];
        mates[k] = hc::srself::Mates{seq + P.off1, qual + P.off1, seq + P.off2, qual + P.off2, P.len1, P.len2};
    }
    self_host_pairs(c, settings, mates, overlap_pos, score, status, W);
    const uint64_t total = self_offsets(W, n_pairs, 0, status, out_off, stats, B.n_offsets);
    *n_out = total;
    if ((rc = hc::sr::check_room("hc_sr_merge_self_overlaps", "merged_seq / merged_qual", "n_out", total, cap, merged_seq, merged_qual))) return rc;
    if (total == 0) return HC_OK;
    if ((rc = S.out_seq.ensure(total)) || (rc = S.out_qual.ensure(total))) return rc;
    if ((rc = self_merge(c, S.seq.as<uint8_t>(), S.qual.as<uint8_t>(), n_pairs, W, total, S.out_seq.as<uint8_t>(), S.out_qual.as<uint8_t>()))) return rc;
    HC_HIP(hipMemcpyAsync(merged_seq, S.out_seq.p, total, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(merged_qual, S.out_qual.p, total, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    if ((rc = self_merge_ms(c, W, stats))) return rc;
    for (size_t k = 0; k < W.host_pairs.size(); k++) {  // the host's pairs are spliced in
        const uint64_t i = W.host_pairs[k].first;
        if (W.host_out[k].seq.empty()) continue;
        memcpy(merged_seq + out_off[i], W.host_out[k].seq.data(), W.host_out[k].seq.size());
        memcpy(merged_qual + out_off[i], W.host_out[k].qual.data(), W.host_out[k].qual.size());
    }
    return HC_OK;
}

// The same from the consensus bytes the context keeps (hc_sr_keep_device): the check runs on the device, the mates of the pairs the host
// decides come back packed in one copy, and the merged reads are appended to the kept bytes without crossing the link.
extern "C" int hc_sr_merge_self_overlaps_kept(hc_ctx* c, const hc_sr_pair* pairs, uint64_t n_pairs, const hc_sr_self_settings* settings,
                                              int32_t* overlap_pos, double* score, uint32_t* status, uint64_t* out_off, uint64_t* n_out,
                                              hc_sr_self_stats* stats) {
    const std::string me = "hc_sr_merge_self_overlaps_kept: ";
    if (!c || !settings || !out_off || !n_out || (n_pairs && (!pairs || !overlap_pos || !score || !status)))
        return fail(HC_ERR_ARG, me + "null argument");
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, me + "min_qual is NaN");
    if (n_pairs >= (1ull << 32) - 1) return fail(HC_ERR_ARG, me + "more than 2^32 - 2 pairs");
    if (!c->srn.keep) return fail(HC_ERR_STATE, me + "hc_sr_keep_device is off");
    if (!c->sr.kept_valid) return fail(HC_ERR_STATE, me + "no kept consensus bytes (hc_sr_consensus, hc_sr_edge_merge or hc_sr_kept_load first)");
    return hc::sr_self_kept_run(c, me.c_str(), pairs, n_pairs, settings, overlap_pos, score, status, out_off, n_out, stats);
}

// hc_sr_merge_self_overlaps_kept behind its checks: hc_sr_merge_next (hc_api_sr_merge_next.cpp) runs the same on the pairs it builds
int hc::sr_self_kept_run(hc_ctx* c, const char* me_, const hc_sr_pair* pairs, uint64_t n_pairs, const hc_sr_self_settings* settings,
                         int32_t* overlap_pos, double* score, uint32_t* status, uint64_t* out_off, uint64_t* n_out, hc_sr_self_stats* stats) {
    const std::string me = me_;
    hc_ctx::Sr& K = c->sr;
    if (stats) memset(stats, 0, sizeof *stats);
    const uint64_t base = K.kept_bytes;
    *n_out = 0;
    out_off[0] = base;
    if (n_pairs == 0) return HC_OK;
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::SrSelf& S = c->sr_self;
    hipStream_t s = c->stream;
    int rc;
    if ((rc = kept_reserve(c, base)) || (rc = S.pairs.ensure(n_pairs * sizeof(hc_sr_pair))) || (rc = S.skip.ensure(n_pairs * sizeof(uint32_t))) ||
        (rc = S.check.ensure(sizeof(hc::SrSelfCheckCounters))))
        return rc;
    // the pairs' checks and the quality values of the batch, on the device
    SelfBatch B;
    B.skip.resize(n_pairs);
    hc::SrSelfCheckCounters cnt;
    float ms_check = 0;
    HC_HIP(hipMemcpyAsync(S.pairs.p, pairs, n_pairs * sizeof(hc_sr_pair), hipMemcpyHostToDevice, s));
    HC_HIP(hipMemsetAsync(S.check.p, 0, sizeof cnt, s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::sr_self_launch_check(K.seq.as<uint8_t>(), K.qual.as<uint8_t>(), base, S.pairs.as<hc_sr_pair>(), n_pairs, settings->min_overlap,
                                    S.skip.as<uint32_t>(), S.check.as<hc::SrSelfCheckCounters>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipMemcpyAsync(B.skip.data(), S.skip.p, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(&cnt, S.check.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_check, c->ev0, c->ev1));
    for (uint32_t q = 33; q <= 126; q++) B.qs_seen[q - 33] = (cnt.qmask[q >> 5] >> (q & 31u)) & 1u;
    B.max_len = cnt.max_len;
    B.max_first = cnt.max_first;
    B.n_offsets = cnt.sum_first;
    B.n_valid = cnt.n_valid;
    if (stats) stats->n_offsets = B.n_offsets;
    SelfWork W;
    self_begin(B, n_pairs, overlap_pos, score, status, W);
    if (B.n_valid && B.max_first &&
        (rc = self_scan(c, me, B, K.seq.as<uint8_t>(), K.qual.as<uint8_t>(), pairs, n_pairs, settings, overlap_pos, score, status, W)))
        return rc;
    W.ms_scan += ms_check;
    // the pairs the host decides: their mates, packed by the copy kernel, in one copy each for bases and qualities
    const size_t n_host = W.host_pairs.size();
    std::vector<hc::SrSelfSeg> segs(n_host);
    std::vector<uint8_t> h_seq, h_qual;
    std::vector<hc::srself::Mates> mates(n_host);
    if (n_host) {
        uint64_t at = 0;
        for (size_t k = 0; k < n_host; k++) {
            const hc_sr_pair& P = pairs[W.host_pairs[k].first];
            segs[k] = hc::SrSelfSeg{P.off1, P.off2, at, P.len1, P.len2};
            at += (uint64_t)P.len1 + P.len2;
        }
        h_seq.resize(at);
        h_qual.resize(at);
        if ((rc = S.segs.ensure(n_host * sizeof(hc::SrSelfSeg))) || (rc = S.stage_seq.ensure(at)) || (rc = S.stage_qual.ensure(at))) return rc;
        HC_HIP(hipMemcpyAsync(S.segs.p, segs.data(), n_host * sizeof(hc::SrSelfSeg), hipMemcpyHostToDevice, s));
        HC_HIP(hc::sr_self_launch_copy(S.segs.as<hc::SrSelfSeg>(), n_host, K.seq.as<uint8_t>(), K.qual.as<uint8_t>(), S.stage_seq.as<uint8_t>(),
                                       S.stage_qual.as<uint8_t>(), s));
        HC_HIP(hipMemcpyAsync(h_seq.data(), S.stage_seq.p, at, hipMemcpyDeviceToHost, s));
        HC_HIP(hipMemcpyAsync(h_qual.data(), S.stage_qual.p, at, hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        for (size_t k = 0; k < n_host; k++) {
            const hc::SrSelfSeg& g = segs[k];
            mates[k] = hc::srself::Mates{h_seq.data() + g.dst, h_qual.data() + g.dst, h_seq.data() + g.dst + g.len1, h_qual.data() + g.dst + g.len1,
                                         g.len1, g.len2};
        }
    }
    self_host_pairs(c, settings, mates, overlap_pos, score, status, W);
    const uint64_t total = self_offsets(W, n_pairs, base, status, out_off, stats, B.n_offsets);
    if (total == 0) return HC_OK;
    // the kept bytes grow, and the merged reads are written straight behind them
    if ((rc = kept_reserve(c, base + total))) return rc;
    if ((rc = self_merge(c, K.seq.as<uint8_t>(), K.qual.as<uint8_t>(), n_pairs, W, total, K.seq.as<uint8_t>() + base, K.qual.as<uint8_t>() + base)))
        return rc;
    // the host's pairs are spliced in: their merged reads go up packed, and the copy kernel puts them in place
    uint64_t n_up = 0, up_bytes = 0;
    for (size_t k = 0; k < n_host; k++) {
        const uint64_t n = W.host_out[k].seq.size();
        if (!n) continue;
        memcpy(h_seq.data() + up_bytes, W.host_out[k].seq.data(), n);  // (a merged read is shorter than its mates together: it fits)
        memcpy(h_qual.data() + up_bytes, W.host_out[k].qual.data(), n);
        segs[n_up++] = hc::SrSelfSeg{up_bytes, 0, out_off[W.host_pairs[k].first], (uint32_t)n, 0};
        up_bytes += n;
    }
    if (n_up) {
        HC_HIP(hipMemcpyAsync(S.segs.p, segs.data(), n_up * sizeof(hc::SrSelfSeg), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.stage_seq.p, h_seq.data(), up_bytes, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.stage_qual.p, h_qual.data(), up_bytes, hipMemcpyHostToDevice, s));
        HC_HIP(hc::sr_self_launch_copy(S.segs.as<hc::SrSelfSeg>(), n_up, S.stage_seq.as<uint8_t>(), S.stage_qual.as<uint8_t>(), K.seq.as<uint8_t>(),
                                       K.qual.as<uint8_t>(), s));
    }
    HC_HIP(hipStreamSynchronize(s));
    if ((rc = self_merge_ms(c, W, stats))) return rc;
    K.kept_bytes = base + total;
    *n_out = total;
    return HC_OK;
}

extern "C" int hc_sr_kept_load(hc_ctx* c, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes) {
    const std::string me = "hc_sr_kept_load: ";
    if (!c || (n_bytes && (!seq || !qual))) return fail(HC_ERR_ARG, me + "null argument");
    if (!c->srn.keep) return fail(HC_ERR_STATE, me + "hc_sr_keep_device is off");
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::Sr& K = c->sr;
    K.kept_valid = false;
    K.kept_bytes = 0;
    int rc = kept_reserve(c, n_bytes);
    if (rc) return rc;
    if (n_bytes) {
        HC_HIP(hipMemcpyAsync(K.seq.p, seq, n_bytes, hipMemcpyHostToDevice, c->stream));
        HC_HIP(hipMemcpyAsync(K.qual.p, qual, n_bytes, hipMemcpyHostToDevice, c->stream));
        HC_HIP(hipStreamSynchronize(c->stream));
    }
    K.kept_bytes = n_bytes;
    K.kept_valid = true;
    return HC_OK;
}

extern "C" int hc_sr_kept_fetch(hc_ctx* c, uint64_t off, uint64_t n, uint8_t* seq, uint8_t* qual, uint64_t* n_kept) {
    const std::string me = "hc_sr_kept_fetch: ";
    if (!c || !n_kept) return fail(HC_ERR_ARG, me + "null argument");
    const hc_ctx::Sr& K = c->sr;
    *n_kept = (c->srn.keep && K.kept_valid) ? K.kept_bytes : 0;
    if (!c->srn.keep || !K.kept_valid) return fail(HC_ERR_STATE, me + "no kept consensus bytes (hc_sr_keep_device, then hc_sr_consensus or hc_sr_kept_load)");
    if (off > K.kept_bytes || n > K.kept_bytes - off) return fail(HC_ERR_ARG, me + "the range does not lie inside the kept bytes");
    if (n == 0) return HC_OK;
    if (!seq || !qual) return fail(HC_ERR_ARG, me + "null buffer");
    HC_HIP(hipSetDevice(c->device));
    HC_HIP(hipMemcpyAsync(seq, K.seq.as<uint8_t>() + off, n, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipMemcpyAsync(qual, K.qual.as<uint8_t>() + off, n, hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    return HC_OK;
}
