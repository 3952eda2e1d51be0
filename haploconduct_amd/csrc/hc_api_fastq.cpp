// hc_api_fastq.cpp — hc_set_reads_from_fastq_text, hc_fastq_fetch and hc_fastq_set_chunk_bytes (include/hcedge.h): the FASTQ files' text
// read on the device into the read store.  The text goes up in chunks through the context's page-locked stations, the newline count of a
// chunk beside the next one's copy (hc_text_kernels.hip); the kernels of hc_fastq_kernels.hip check the records, read the plain ids and
// gather the raw arrays; from the histograms on it is hc_sr_set_next_reads' tail: plan_store, release_store, finish_store (hc_api.cpp).
// What stays the host's is the host reader's own code (host/host_model.cpp): the --IDs map, the tokens that are not plain, and the text
// of every error, which is made by the reader's checks on the one record the device names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "hc_ctx.h"
#include "hc_fastq.h"
#include "hc_prims.h"
#include "hc_sr_next.h"
#include "hc_text.h"
#include "host/FastqStorage.h"

static int fail(int status, const std::string& what) { return hc::set_last_error(status, what); }

namespace {
const char* const kMe = "hc_set_reads_from_fastq_text: ";
const uint64_t kTile = 4096;
const uint64_t kDefaultChunk = 32ull << 20;        // what hc_set_found_from_sfo_text uses
const uint64_t kMaxFileBytes = (1ull << 32) - kTile;  // line starts are 32-bit offsets (hcedge.h)
constexpr int kStations = 3;

// as hc_host_fastq_load reports a reader's failure (host/api_helpers.h: guarded)
int fail_as_reader(const hc::FatalError& e) { return fail(e.status, std::string("FastqStorage: ") + e.what); }

void parallel_copy(char* dst, const char* src, size_t len, unsigned T) {
    if (T <= 1 || len < (1u << 20)) {
        memcpy(dst, src, len);
        return;
    }
    auto slice = [=](unsigned t) {
        const size_t a = (len * t / T) & ~(size_t)63, e = t + 1 == T ? len : (len * (t + 1) / T) & ~(size_t)63;
        if (e > a) memcpy(dst + a, src + a, e - a);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back(slice, t);
    slice(0);
    for (auto& x : th) x.join();
}

struct File {
    const char* p = nullptr;
    uint64_t n = 0;
    uint32_t n_tiles = 0, n_newlines = 0, n_rec = 0;  // n_rec: records the reader takes of this file alone
};

// the four lines of the record whose header starts at `at`, as LineFile::next4 yields them
void record_lines(const File& f, uint64_t at, const char* l[4], size_t n[4]) {
    const char* q = f.p + at;
    const char* const e = f.p + f.n;
    for (int k = 0; k < 4; k++) {
        const char* nl = q < e ? (const char*)memchr(q, '\n', (size_t)(e - q)) : nullptr;
        l[k] = q;
        n[k] = nl ? (size_t)(nl - q) : (size_t)(e - q);
        q = nl ? nl + 1 : e;
    }
}

struct Streams {  // this call's own
    hipStream_t copy = nullptr;
    hipEvent_t copied[kStations] = {};
    ~Streams() {
        for (hipEvent_t e : copied)
            if (e) (void)hipEventDestroy(e);
        if (copy) (void)hipStreamDestroy(copy);
    }
};
}  // namespace

extern "C" int hc_fastq_set_chunk_bytes(hc_ctx* c, uint64_t bytes) {
    if (!c) return fail(HC_ERR_ARG, "hc_fastq_set_chunk_bytes: null context");
    if (bytes && bytes < kTile) return fail(HC_ERR_ARG, "hc_fastq_set_chunk_bytes: a chunk has 4096 bytes at least");
    c->fastq.chunk_bytes = bytes;
    return HC_OK;
}

extern "C" int hc_fastq_fetch(hc_ctx* c, uint64_t* read_ids, uint64_t cap_reads, uint64_t* seq_off, uint32_t* read_first_seq, uint64_t cap_seq) {
    const char* me = "hc_fastq_fetch: ";
    if (!c) return fail(HC_ERR_ARG, std::string(me) + "null context");
    const hc_ctx::Fastq& F = c->fastq;
    if (!F.valid) return fail(HC_ERR_STATE, std::string(me) + "no store read by hc_set_reads_from_fastq_text");
    if (!read_ids || !seq_off || !read_first_seq || cap_reads < F.read_ids.size() || cap_seq + 1 < F.seq_off.size())
        return fail(HC_ERR_ARG, std::string(me) + "a buffer is missing or too small (the call's counts hold the need)");
    if (!F.read_ids.empty()) memcpy(read_ids, F.read_ids.data(), F.read_ids.size() * sizeof(uint64_t));
    memcpy(seq_off, F.seq_off.data(), F.seq_off.size() * sizeof(uint64_t));
    memcpy(read_first_seq, F.first.data(), F.first.size() * sizeof(uint32_t));
    return HC_OK;
}

extern "C" int hc_set_reads_from_fastq_text(hc_ctx* c, const hc_fastq_text* tx, hc_fastq_counts* counts) {
    if (!c || !tx || !counts) return fail(HC_ERR_ARG, std::string(kMe) + "null argument");
    if ((tx->n_singles && !tx->singles) || (tx->n_paired1 && !tx->paired1) || (tx->n_paired2 && !tx->paired2))
        return fail(HC_ERR_ARG, std::string(kMe) + "a text without its bytes");
    hc_fastq_counts cn;
    memset(&cn, 0, sizeof cn);
    cn.err_file = -1;
    *counts = cn;
    if (c->settings.device_mask & ~(1u << c->device))
        return fail(HC_ERR_NOT_ON_DEVICE, std::string(kMe) + "not on the device (the stage scores on several devices)");
    File file[3];
    file[0].p = tx->singles, file[0].n = tx->singles ? tx->n_singles : 0;
    file[1].p = tx->paired1, file[1].n = tx->paired1 ? tx->n_paired1 : 0;
    file[2].p = tx->paired2, file[2].n = tx->paired2 ? tx->n_paired2 : 0;
    for (const File& f : file)
        if (f.n >= kMaxFileBytes) return fail(HC_ERR_NOT_ON_DEVICE, std::string(kMe) + "not on the device (a file of 2^32 - 4096 bytes and more)");
    // the --IDs map first, as the reader's constructor reads it in front of the files
    std::unique_ptr<hc::FastqStorage> idmap;
    const bool have_map = tx->ids_path != nullptr;
    try {
        idmap.reset(new hc::FastqStorage(hc::FastqStorage::IdsOnly{}, have_map ? std::string(tx->ids_path) : std::string()));
    } catch (const hc::FatalError& e) {
        return fail_as_reader(e);
    } catch (const std::exception& e) {
        return fail(HC_ERR_FORMAT, std::string("FastqStorage: ") + e.what());
    }
    HC_HIP(hipSetDevice(c->device));
    hc_ctx::Fastq& F = c->fastq;
    hipStream_t st = c->stream;
    const uint64_t max_lines = 4ull * (unsigned int)tx->max_reads;
    uint64_t chunk = (F.chunk_bytes ? F.chunk_bytes : kDefaultChunk) & ~(kTile - 1);
    int rc;

    // ---- upload: chunk k + 1's copy beside chunk k's newline count --------------------------------------------------------
    const auto t_copy = std::chrono::steady_clock::now();
    Streams S;
    HC_HIP(hipStreamCreateWithFlags(&S.copy, hipStreamNonBlocking));
    for (hipEvent_t& e : S.copied) HC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint64_t largest = 0;
    for (const File& f : file) largest = std::max(largest, f.n);
    for (hc_scratch& h : c->h_sfo_text)
        if ((rc = h.ensure_exact(std::min(chunk, std::max<uint64_t>(largest, kTile)) + 64))) return rc;
    unsigned T = std::thread::hardware_concurrency();
    T = T == 0 ? 1 : (T > 16 ? 16 : T);
    uint64_t k = 0;  // chunks so far, over the files: the stations take turns
    uint32_t max_tiles = 0;
    for (int i = 0; i < 3; i++) {
        File& f = file[i];
        f.n_tiles = (uint32_t)((f.n + kTile - 1) / kTile);
        max_tiles = std::max(max_tiles, f.n_tiles);
        if (f.n == 0) continue;
        if ((rc = F.text[i].ensure(f.n + 64)) || (rc = F.tiles[i].ensure(((size_t)f.n_tiles + 1) * sizeof(uint32_t)))) return rc;
        for (uint64_t pos = 0; pos < f.n; pos += chunk, k++) {
            const uint64_t len = std::min(chunk, f.n - pos);
            const int j = (int)(k % kStations);
            if (k >= (uint64_t)kStations) HC_HIP(hipEventSynchronize(S.copied[j]));  // the station's buffer has left for the device
            parallel_copy(c->h_sfo_text[j].as<char>(), f.p + pos, (size_t)len, f.n < (8u << 20) ? 1u : T);
            HC_HIP(hipMemcpyAsync(F.text[i].as<char>() + pos, c->h_sfo_text[j].p, len, hipMemcpyHostToDevice, S.copy));
            HC_HIP(hipEventRecord(S.copied[j], S.copy));
            HC_HIP(hipStreamWaitEvent(st, S.copied[j], 0));
            // (pos is a whole number of tiles; a piece that reaches past the chunk's end is masked: hc_text_kernels.hip)
            HC_HIP(hc::launch_text_count(F.text[i].as<char>() + pos, len, F.tiles[i].as<uint32_t>() + pos / kTile, st));
        }
    }
    const size_t scan_tiles = hc::prims::scan_temp_bytes((uint64_t)max_tiles + 1, sizeof(uint32_t));
    if ((rc = F.temp.ensure(scan_tiles ? scan_tiles : 16)) || (rc = F.counters.ensure(8 * sizeof(unsigned long long)))) return rc;
    uint32_t newlines[3] = {0, 0, 0};
    for (int i = 0; i < 3; i++) {
        if (file[i].n == 0) continue;
        uint32_t* tiles = F.tiles[i].as<uint32_t>();
        HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, tiles, tiles, (uint64_t)file[i].n_tiles + 1, st));
        HC_HIP(hipMemcpyAsync(&newlines[i], tiles + file[i].n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HC_HIP(hipStreamSynchronize(st));
    HC_HIP(hipStreamSynchronize(S.copy));
    cn.ms_copy = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_copy).count();
    for (int i = 0; i < 3; i++) {
        File& f = file[i];
        f.n_newlines = newlines[i];
        const uint64_t lines = f.n ? (uint64_t)f.n_newlines + (f.p[f.n - 1] != '\n' ? 1u : 0u) : 0;
        f.n_rec = (uint32_t)(std::min(lines, max_lines) / 4);  // an incomplete last record is ignored
    }
    const uint32_t n_single = file[0].n_rec, n_paired = tx->paired1 ? std::min(file[1].n_rec, file[2].n_rec) : 0u;  // up to the shorter file
    const uint64_t n_reads64 = (uint64_t)n_single + n_paired, n_seq64 = (uint64_t)n_single + 2ull * n_paired;
    if (n_seq64 > 0xFFFFFFFFull) return fail(HC_ERR_BAD_READ, "hc_set_reads: more than 2^32 - 1 sequences");
    const uint32_t n_reads = (uint32_t)n_reads64, n_seq = (uint32_t)n_seq64;
    const uint32_t n_used[3] = {n_single, n_paired, n_paired};

    // ---- lines, records, lengths ---------------------------------------------------------------------------------------
    const size_t scan_seq = hc::prims::scan_temp_bytes((uint64_t)n_seq + 1, sizeof(uint64_t));
    const size_t per_read = n_reads ? n_reads : 1;
    if ((rc = F.temp.ensure(std::max(scan_seq, scan_tiles) ? std::max(scan_seq, scan_tiles) : 16)) || (rc = F.ids.ensure(per_read * sizeof(uint64_t))) ||
        (rc = F.tok_off.ensure(per_read * sizeof(uint32_t))) || (rc = F.tok_len.ensure(per_read * sizeof(uint32_t))) ||
        (rc = F.not_plain.ensure(per_read)) || (rc = F.lens.ensure(((size_t)n_seq + 1) * sizeof(uint64_t))) ||
        (rc = F.off.ensure(((size_t)n_seq + 1) * sizeof(uint64_t))) || (rc = F.hist.ensure(512 * sizeof(unsigned long long))))
        return rc;
    hc::FastqFile dev[3];
    for (int i = 0; i < 3; i++) {
        if ((rc = F.line_start[i].ensure((4 * (size_t)n_used[i] + 1) * sizeof(uint32_t)))) return rc;
        dev[i] = hc::FastqFile{F.text[i].as<char>(), F.line_start[i].as<uint32_t>(), file[i].n, file[i].n_newlines};
    }
    unsigned long long* const d_cnt = F.counters.as<unsigned long long>();  // first bad of the singles, of the pairs; tokens not plain; bytes
    HC_HIP(hipMemsetAsync(d_cnt, 0xFF, 2 * sizeof(unsigned long long), st));
    HC_HIP(hipMemsetAsync(d_cnt + 2, 0, 2 * sizeof(unsigned long long), st));
    HC_HIP(hipEventRecord(c->ev0, st));
    for (int i = 0; i < 3; i++)
        if (n_used[i])
            HC_HIP(hc::launch_text_line_starts(dev[i].text, dev[i].n_bytes, F.tiles[i].as<uint32_t>(), 4u * n_used[i], F.line_start[i].as<uint32_t>(), st));
    const hc::FastqRecordsOut out_s{F.ids.as<uint64_t>(), F.tok_off.as<uint32_t>(), F.tok_len.as<uint32_t>(), F.not_plain.as<uint8_t>(),
                                    F.lens.as<uint64_t>(), d_cnt, d_cnt + 2};
    hc::FastqRecordsOut out_p = out_s;
    out_p.first_bad = d_cnt + 1;
    HC_HIP(hc::fastq_launch_records(dev[0], dev[0], false, n_single, 0, 0, out_s, st));
    HC_HIP(hc::fastq_launch_records(dev[1], dev[2], true, n_paired, n_single, n_single, out_p, st));
    HC_HIP(hc::prims::exclusive_sum(F.temp.p, F.temp.cap, F.lens.as<uint64_t>(), F.off.as<uint64_t>(), (uint64_t)n_seq + 1, st));
    HC_HIP(hipEventRecord(c->ev1, st));
    unsigned long long h_cnt[3] = {hc::kFastqNoBad, hc::kFastqNoBad, 0};
    uint64_t total = 0;
    HC_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    HC_HIP(hipMemcpyAsync(&total, F.off.as<uint64_t>() + n_seq, sizeof total, hipMemcpyDeviceToHost, st));
    std::vector<uint64_t> ids(n_reads);
    if (n_reads) HC_HIP(hipMemcpyAsync(ids.data(), F.ids.p, (size_t)n_reads * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
    float ms_a = 0, ms_b = 0;
    HC_HIP(hipEventElapsedTime(&ms_a, c->ev0, c->ev1));

    // ---- the host's part of the ids, and the first bad record -----------------------------------------------------------
    // In file order: the singles, then the pairs.  Of a file's records in front of the first one the device refused, the host resolves the
    // tokens the device left to it (every token with an --IDs map): a token that does not resolve there is check 3 of an earlier record.
    // The refused record itself goes through the reader's own checks, which make the status and the text.
    const bool any_host = have_map || h_cnt[2] != 0;
    std::vector<uint32_t> tok_off, tok_len;
    std::vector<uint8_t> not_plain;
    if (any_host && n_reads) {
        tok_off.resize(n_reads), tok_len.resize(n_reads), not_plain.resize(n_reads);
        HC_HIP(hipMemcpy(tok_off.data(), F.tok_off.p, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HC_HIP(hipMemcpy(tok_len.data(), F.tok_len.p, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HC_HIP(hipMemcpy(not_plain.data(), F.not_plain.p, (size_t)n_reads, hipMemcpyDeviceToHost));
    }
    uint64_t n_host_ids = 0;
    for (int part = 0; part < 2; part++) {
        const bool paired = part == 1;
        const File& f1 = file[paired ? 1 : 0];
        const uint32_t n = paired ? n_paired : n_single, first_read = paired ? n_single : 0u;
        const bool refused = h_cnt[part] != hc::kFastqNoBad;
        const uint32_t upto = refused ? (uint32_t)(h_cnt[part] >> 3) : n;
        if (any_host && upto) {
            const unsigned W = upto < 65536 ? 1u : T;
            std::vector<uint64_t> bad_at(W, ~0ull), resolved(W, 0);
            std::vector<hc::FatalError> err(W, hc::FatalError{0, ""});
            auto work = [&](unsigned t) {
                for (uint64_t r = (uint64_t)upto * t / W; r < (uint64_t)upto * (t + 1) / W; r++) {
                    const uint32_t read = first_read + (uint32_t)r;
                    if (!have_map && !not_plain[read]) continue;
                    try {
                        ids[read] = idmap->resolve_token(f1.p + tok_off[read], tok_len[read]);
                        resolved[t]++;
                    } catch (const hc::FatalError& e) {
                        bad_at[t] = r, err[t] = e;
                        return;
                    }
                }
            };
            std::vector<std::thread> th;
            for (unsigned t = 1; t < W; t++) th.emplace_back(work, t);
            work(0);
            for (auto& x : th) x.join();
            for (unsigned t = 0; t < W; t++) {
                if (bad_at[t] != ~0ull) {  // the threads own ascending ranges
                    cn.err_file = part, cn.err_record = bad_at[t];
                    *counts = cn;
                    return fail_as_reader(err[t]);
                }
                n_host_ids += resolved[t];
            }
        }
        if (refused) {
            const uint64_t r = upto;
            uint32_t at[2] = {0, 0};
            HC_HIP(hipMemcpy(&at[0], F.line_start[paired ? 1 : 0].as<uint32_t>() + 4 * r, sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (paired) HC_HIP(hipMemcpy(&at[1], F.line_start[2].as<uint32_t>() + 4 * r, sizeof(uint32_t), hipMemcpyDeviceToHost));
            const char *l1[4], *l2[4] = {nullptr, nullptr, nullptr, nullptr};
            size_t n1[4], n2[4] = {0, 0, 0, 0};
            record_lines(f1, at[0], l1, n1);
            if (paired) record_lines(file[2], at[1], l2, n2);
            cn.err_file = part, cn.err_record = r;
            *counts = cn;
            try {
                (void)idmap->check_record(l1, n1, l2, n2, paired);
            } catch (const hc::FatalError& e) {
                return fail_as_reader(e);
            }
            return fail(HC_ERR_STATE, std::string(kMe) + "the device refused a record the reader's checks accept");
        }
    }

    // ---- what hc_set_reads refuses ------------------------------------------------------------------------------------------
    std::vector<uint64_t> h_off((size_t)n_seq + 1, 0);
    if (n_seq) HC_HIP(hipMemcpy(h_off.data(), F.off.p, h_off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    hc::StorePlan P;
    P.seq_len.resize(n_seq ? n_seq : 1);
    for (uint32_t q = 0; q < n_seq; q++) {
        const uint64_t len = h_off[q + 1] - h_off[q];
        if (len >= (1ull << 28)) return fail(HC_ERR_BAD_READ, "hc_set_reads: sequence longer than 2^28-1");
        P.seq_len[q] = (uint32_t)len;
    }
    P.total = total;
    std::vector<uint32_t> h_first((size_t)n_reads + 1);
    for (uint32_t r = 0; r <= n_reads; r++) h_first[r] = r <= n_single ? r : n_single + 2u * (r - n_single);

    // ---- gather, histograms, and hc_sr_set_next_reads' tail ----------------------------------------------------------------
    hc_ctx::SrNext& N = c->srn;
    hc_scratch t_bases, t_quals, t_off, t_first;  // this call's own, unless the raw arrays are kept
    hc_scratch &s_bases = N.keep ? N.next_bases : t_bases, &s_quals = N.keep ? N.next_quals : t_quals, &s_off = N.keep ? N.next_off : t_off,
               &s_first = N.keep ? N.next_first : t_first;
    if (N.keep) {  // the next_* blocks are about to be overwritten (hc_api_sr_next.cpp: sr_next_store)
        N.prev_clear();
        c->sr_fastq.drop();
    }
    if ((rc = s_bases.ensure_exact(total ? total : 1)) || (rc = s_quals.ensure_exact(total ? total : 1)) ||
        (rc = s_off.ensure_exact(sizeof(uint64_t) * ((size_t)n_seq + 1))) || (rc = s_first.ensure_exact(sizeof(uint32_t) * ((size_t)n_reads + 1))))
        return rc;
    HC_HIP(hipMemsetAsync(F.hist.p, 0, 512 * sizeof(unsigned long long), st));
    HC_HIP(hipMemcpyAsync(s_off.p, F.off.p, sizeof(uint64_t) * ((size_t)n_seq + 1), hipMemcpyDeviceToDevice, st));
    HC_HIP(hipMemcpyAsync(s_first.p, h_first.data(), sizeof(uint32_t) * h_first.size(), hipMemcpyHostToDevice, st));
    HC_HIP(hipEventRecord(c->ev0, st));
    hc::FastqGather G{{dev[0], dev[1], dev[2]}, n_single, n_seq, s_off.as<uint64_t>(), s_bases.as<uint8_t>(), s_quals.as<uint8_t>()};
    HC_HIP(hc::fastq_launch_gather(G, st));
    HC_HIP(hc::fastq_launch_upper(s_bases.as<uint8_t>(), h_off[n_single], c->n_cu, st));  // singles only: boost::to_upper_copy, :122
    if (total) HC_HIP(hc::sr_next_launch_hist(s_bases.as<uint8_t>(), s_quals.as<uint8_t>(), total, c->n_cu, F.hist.as<unsigned long long>(), st));
    HC_HIP(hipEventRecord(c->ev1, st));
    unsigned long long hist[512];
    HC_HIP(hipMemcpyAsync(hist, F.hist.p, sizeof hist, hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
    HC_HIP(hipEventElapsedTime(&ms_b, c->ev0, c->ev1));
    cn.ms_device = (double)ms_a + (double)ms_b;
    const auto t_plan = std::chrono::steady_clock::now();
    uint64_t qh[256], bh[256];
    for (int b = 0; b < 256; b++) {
        qh[b] = hist[b];
        bh[b] = hist[256 + b];
    }
    if ((rc = hc::plan_store(c, qh, bh, h_first.data(), n_reads, P))) return rc;
    cn.ms_plan = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan).count();
    hc::release_store(c);
    N.raw_valid = false;
    if ((rc = hc::finish_store(c, P, s_bases.as<uint8_t>(), s_quals.as<uint8_t>(), s_off.as<uint64_t>(), s_first.as<uint32_t>(), h_first.data(), n_reads)))
        return rc;
    if (N.keep) {  // the new raw arrays become the kept ones, as hc_set_reads leaves them: nothing of the old store stays
        N.bases.swap(N.next_bases);
        N.quals.swap(N.next_quals);
        N.off.swap(N.next_off);
        N.first.swap(N.next_first);
        for (hc_scratch* b : {&N.next_bases, &N.next_quals, &N.next_off, &N.next_first}) b->release();
        N.h_off = h_off;
        N.h_first = h_first;
        N.total = total;
        N.raw_valid = true;
    }
    cn.n_reads = n_reads, cn.n_seq = n_seq, cn.n_single = n_single, cn.n_paired = n_paired;
    cn.n_bytes = total;
    cn.n_host_ids = n_host_ids;
    F.read_ids.swap(ids);
    F.seq_off.swap(h_off);
    F.first.swap(h_first);
    F.counts = cn;
    F.valid = true;
    *counts = cn;
    return HC_OK;
}
