// hc_api_sr.cpp — hc_sr_consensus (include/hcsr.h): SRBuilder::consensus / consensus_pos (reference src/SRBuilder.cpp:289-535) for a
// batch of layouts on the device.  The host builds what depends on libm — the per-quality log10 terms and the table of one- and
// two-member columns, once per read set and min_qual —, the kernels of hc_sr_kernels.hip do the rest, and the columns they could not
// decide by comparisons come back as four sums that host threads finish with the reference's expressions (host/SrConsensus.h).
// hc_sr_consensus is in parts (hc_ctx.h: sr_consensus_begin / _room / _run) so that hc_sr_edge_merge (hc_api_sr_edge.cpp), whose layouts are
// on the device already, runs the same code from there on.
// hc_sr_merge_self_overlaps: SRBuilder::merge_self_overlap (:872-955) for a batch of pairs, at the end of this file.  Both calls build
// their consensus tables with sr_tables and run their host loops with in_blocks (host/InBlocks.h).
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
#include "hc_sr_next.h"
#include "hc_sr_self.h"
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
// hc_sr_merge_self_overlaps: the host checks the pairs and builds what depends on libm (the log p table of the batch's quality values, by
// the scoring path's own builder; 1.0 / n; the consensus table), the scan kernel finds every pair's offset, the host decides the offsets
// inside the guard band (host/SrSelfOverlap.h), the merge kernel writes the merged reads at the offsets of an exclusive sum.
extern "C" int hc_sr_merge_self_overlaps(hc_ctx* c, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes, const hc_sr_pair* pairs,
                                         uint64_t n_pairs, const hc_sr_self_settings* settings, int32_t* overlap_pos, double* score,
                                         uint32_t* status, uint64_t* out_off, uint8_t* merged_seq, uint8_t* merged_qual, uint64_t cap,
                                         uint64_t* n_out, hc_sr_self_stats* stats) {
    const char* me = "hc_sr_merge_self_overlaps: ";
    if (!c || !settings || !out_off || !n_out || (n_pairs && (!pairs || !overlap_pos || !score || !status)) || (n_bytes && (!seq || !qual)))
        return fail(HC_ERR_ARG, std::string(me) + "null argument");
    if (!(settings->min_qual == settings->min_qual)) return fail(HC_ERR_ARG, std::string(me) + "min_qual is NaN");
    if (n_pairs >= (1ull << 32) - 1) return fail(HC_ERR_ARG, std::string(me) + "more than 2^32 - 2 pairs");
    if (stats) memset(stats, 0, sizeof *stats);
    *n_out = 0;
    out_off[0] = 0;
    if (n_pairs == 0) return HC_OK;
    HC_HIP(hipSetDevice(c->device));
    const auto t_host0 = std::chrono::steady_clock::now();
    double ms_host = 0;
    const unsigned n_thr = std::max(1u, settings->n_threads);
    // the pairs' checks and the quality values of the batch
    std::vector<uint32_t> skip(n_pairs);
    const uint64_t check_block = 1024, n_check_blocks = (n_pairs + check_block - 1) / check_block;
    std::vector<std::array<uint8_t, 128>> seen(n_check_blocks);
    std::vector<uint32_t> block_max(n_check_blocks, 0);
    hc::in_blocks(n_pairs, check_block, n_thr, [&](uint64_t a, uint64_t b) {
        std::array<uint8_t, 128>& sn = seen[a / check_block];
        sn.fill(0);
        uint32_t mx = 0;
        for (uint64_t i = a; i < b; i++) {
            skip[i] = hc::srself::check_pair(seq, qual, n_bytes, pairs[i]);
            if (skip[i]) continue;
            const hc_sr_pair& P = pairs[i];
            for (uint32_t k = 0; k < P.len1; k++) sn[qual[P.off1 + k] & 127u] = 1;
            for (uint32_t k = 0; k < P.len2; k++) sn[qual[P.off2 + k] & 127u] = 1;
            mx = std::max({mx, P.len1, P.len2});
        }
        block_max[a / check_block] = mx;
    });
    uint32_t max_len = 0, max_first = 0;
    uint64_t n_offsets = 0, n_valid = 0;
    uint8_t qs_seen[96] = {0};
    for (uint64_t b = 0; b < n_check_blocks; b++) {
        max_len = std::max(max_len, block_max[b]);
        for (uint32_t q = 33; q <= 126; q++) qs_seen[q - 33] |= seen[b][q];
    }
    for (uint64_t i = 0; i < n_pairs; i++) {
        overlap_pos[i] = -1;
        score[i] = 0;
        status[i] = skip[i];
        if (skip[i]) continue;
        n_valid++;
        const uint32_t f = hc::srself::first_offset(pairs[i].len1, settings->min_overlap);
        n_offsets += f;
        max_first = std::max(max_first, f);
    }
    if (stats) stats->n_offsets = n_offsets;
    hc_ctx::SrSelf& S = c->sr_self;
    hipStream_t s = c->stream;
    std::vector<hc::SrSelfScan> res(n_pairs);
    std::vector<uint64_t> len(n_pairs + 1, 0);
    std::vector<int32_t> mpos(n_pairs, -1);
    // pairs the host finishes: (pair, the offset its scan goes on from)
    std::vector<std::pair<uint64_t, uint32_t>> host_pairs;
    float ms_scan = 0, ms_merge = 0;
    int rc = HC_OK;
    if (n_valid && max_first) {
        // tables: log p by the scoring path's builder for the batch's values (row = rank of the value), 1.0 / n, the consensus table
        std::vector<int> phred;
        uint8_t qmap[256], q_of[hc::sr::kQDim];
        memset(qmap, 0, sizeof qmap);
        memset(q_of, 255, sizeof q_of);
        for (uint32_t q = 0; q < hc::srself::kQ; q++) {
            if (!qs_seen[q]) continue;
            qmap[q + 33] = (uint8_t)phred.size();
            phred.push_back((int)q);
            q_of[q] = (uint8_t)q;
        }
        std::vector<double> lut;
        if (!hc::build_log_table_u16(phred, c->settings.mismatch, lut)) return fail(HC_ERR_STATE, std::string(me) + "the log table is not symmetric");
        std::vector<double> inv_n((size_t)max_len + 1, 0.0);
        for (uint32_t k = 1; k <= max_len; k++) inv_n[k] = 1.0 / (double)k;  // :137
        if ((rc = sr_tables(c, S.tables, q_of, settings->min_qual))) return rc;
        hc::SrSelfParams prm;
        int log2_width = -49;
        if (const char* e = getenv("HC_SR_SELF_BAND_LOG2")) {  // test knob: a wider guard band, so that the host-decided path runs
            const int v = atoi(e);
            if (v >= -60 && v <= -2) log2_width = v;
        }
        prm.band = hc::threshold_band(settings->min_score, log2_width);
        prm.always = settings->min_score < 0 ? 1u : 0u;
        prm.min_overlap = settings->min_overlap;
        prm.min_read_len = c->settings.min_read_len;
        prm.K = (uint32_t)phred.size();
        prm.lut_doubles = (uint32_t)lut.size();
        prm.inv_len = (uint32_t)inv_n.size();
        const size_t scan_bytes = hc::prims::scan_temp_bytes(n_pairs + 1, sizeof(uint64_t));
        if ((rc = S.seq.ensure(n_bytes)) || (rc = S.qual.ensure(n_bytes)) || (rc = S.pairs.ensure(n_pairs * sizeof(hc_sr_pair))) ||
            (rc = S.skip.ensure(n_pairs * sizeof(uint32_t))) || (rc = S.qmap.ensure(256)) || (rc = S.lut.ensure(lut.size() * sizeof(double))) ||
            (rc = S.inv_n.ensure(inv_n.size() * sizeof(double))) || (rc = S.res.ensure(n_pairs * sizeof(hc::SrSelfScan))) ||
            (rc = S.len.ensure((n_pairs + 1) * sizeof(uint64_t))) || (rc = S.off.ensure((n_pairs + 1) * sizeof(uint64_t))) ||
            (rc = S.mpos.ensure(n_pairs * sizeof(int32_t))) || (rc = S.temp.ensure(scan_bytes ? scan_bytes : 16)))
            return rc;
        ms_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
        HC_HIP(hipMemcpyAsync(S.seq.p, seq, n_bytes, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.qual.p, qual, n_bytes, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.pairs.p, pairs, n_pairs * sizeof(hc_sr_pair), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.skip.p, skip.data(), n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.qmap.p, qmap, 256, hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.lut.p, lut.data(), lut.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HC_HIP(hipMemcpyAsync(S.inv_n.p, inv_n.data(), inv_n.size() * sizeof(double), hipMemcpyHostToDevice, s));
        const uint32_t lanes = 64u * std::max(1u, std::min(hc::kSelfMaxChunk / 64u, (max_first + 63u) / 64u));
        HC_HIP(hipEventRecord(c->ev0, s));
        HC_HIP(hc::sr_self_launch_scan(c->n_cu, lanes, S.seq.as<uint8_t>(), S.qual.as<uint8_t>(), S.pairs.as<hc_sr_pair>(), S.skip.as<uint32_t>(), n_pairs,
                                       S.qmap.as<uint8_t>(), S.lut.as<double>(), S.inv_n.as<double>(), prm, S.res.as<hc::SrSelfScan>(), s));
        HC_HIP(hipEventRecord(c->ev1, s));
        HC_HIP(hipMemcpyAsync(res.data(), S.res.p, n_pairs * sizeof(hc::SrSelfScan), hipMemcpyDeviceToHost, s));
        HC_HIP(hipStreamSynchronize(s));
        HC_HIP(hipEventElapsedTime(&ms_scan, c->ev0, c->ev1));
        for (uint64_t i = 0; i < n_pairs; i++) {
            if (skip[i] || res[i].p < 0) continue;
            if (res[i].kind == hc::kSelfHit && !S.tables.has_nan) {
                overlap_pos[i] = res[i].p;
                score[i] = exp(res[i].x);  // :138
                status[i] = HC_SR_SELF_MERGED;
                len[i] = (uint64_t)pairs[i].len2 + (uint32_t)res[i].p;  // :890
                mpos[i] = res[i].p;
            } else {
                host_pairs.emplace_back(i, (uint32_t)res[i].p);
            }
        }
    }
    // the host's share: the scan goes on from the offset in the band with the host's libm, as the mirror walks it
    struct HostOut {
        std::vector<uint8_t> seq, qual;
    };
    std::vector<HostOut> host_out(host_pairs.size());
    if (!host_pairs.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        const hc::srself::Tables T(c->settings.mismatch, c->settings.min_read_len);
        hc::in_blocks(host_pairs.size(), 1, n_thr, [&](uint64_t a, uint64_t b) {
            for (uint64_t k = a; k < b; k++) {
                const uint64_t i = host_pairs[k].first;
                const hc_sr_pair& P = pairs[i];
                const hc::srself::Mates M{seq + P.off1, qual + P.off1, seq + P.off2, qual + P.off2, P.len1, P.len2};
                overlap_pos[i] = hc::srself::scan_pair(T, M, host_pairs[k].second, *settings, &score[i], host_out[k].seq, host_out[k].qual);
                if (overlap_pos[i] < 0) continue;
                status[i] = HC_SR_SELF_MERGED;
                len[i] = host_out[k].seq.size();
            }
        });
        ms_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    uint64_t total = 0, n_merged = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        out_off[i] = total;
        total += len[i];
        n_merged += status[i] == HC_SR_SELF_MERGED;
    }
    out_off[n_pairs] = total;
    *n_out = total;
    if (stats) {
        stats->n_merged = n_merged;
        stats->n_host_pairs = host_pairs.size();
        stats->ms_device = ms_scan;
        stats->ms_host = ms_host;
    }
    if ((rc = hc::sr::check_room("hc_sr_merge_self_overlaps", "merged_seq / merged_qual", "n_out", total, cap, merged_seq, merged_qual))) return rc;
    if (total == 0) return HC_OK;
    // the merged reads: offsets by an exclusive sum on the device, one lane per column
    if ((rc = S.out_seq.ensure(total)) || (rc = S.out_qual.ensure(total))) return rc;
    HC_HIP(hipMemcpyAsync(S.len.p, len.data(), (n_pairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HC_HIP(hipMemcpyAsync(S.mpos.p, mpos.data(), n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HC_HIP(hipEventRecord(c->ev0, s));
    HC_HIP(hc::prims::exclusive_sum(S.temp.p, S.temp.cap, S.len.as<uint64_t>(), S.off.as<uint64_t>(), n_pairs + 1, s));
    HC_HIP(hc::sr_self_launch_merge(S.seq.as<uint8_t>(), S.qual.as<uint8_t>(), S.pairs.as<hc_sr_pair>(), n_pairs, S.mpos.as<int32_t>(),
                                    S.off.as<uint64_t>(), total, S.tables.terms.as<double>(), S.tables.table.as<uint8_t>(), S.out_seq.as<uint8_t>(),
                                    S.out_qual.as<uint8_t>(), s));
    HC_HIP(hipEventRecord(c->ev1, s));
    HC_HIP(hipMemcpyAsync(merged_seq, S.out_seq.p, total, hipMemcpyDeviceToHost, s));
    HC_HIP(hipMemcpyAsync(merged_qual, S.out_qual.p, total, hipMemcpyDeviceToHost, s));
    HC_HIP(hipStreamSynchronize(s));
    HC_HIP(hipEventElapsedTime(&ms_merge, c->ev0, c->ev1));
    for (size_t k = 0; k < host_pairs.size(); k++) {  // the host's pairs are spliced in
        const uint64_t i = host_pairs[k].first;
        if (host_out[k].seq.empty()) continue;
        memcpy(merged_seq + out_off[i], host_out[k].seq.data(), host_out[k].seq.size());
        memcpy(merged_qual + out_off[i], host_out[k].qual.data(), host_out[k].qual.size());
    }
    if (stats) stats->ms_device = (double)ms_scan + ms_merge;
    return HC_OK;
}
