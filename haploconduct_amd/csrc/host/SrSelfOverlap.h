// SrSelfOverlap.h — SRBuilder::merge_self_overlap (reference src/SRBuilder.cpp:872-955) for one pair with the host's libm: the check of a
// pair, EdgeCalculator::overlap_score (src/EdgeCalculator.cpp:26-139) at one offset, the two-member consensus of the mates and the scan
// over the offsets.  Shared by the host mirror (SrSelfOverlap.cpp) and the device call's glue (hc_api_sr.cpp: the pairs the host decides).
// Own text; the expressions are the reference's, operation for operation.
//
// Why overlap_score is restated here and not called: the project's EdgeCalculator::overlap_score (host/EdgeCalculator.cpp) creates a device
// context and scores the pair with hc_score_batch, so it needs a GPU and costs a context per call.  The mirror has to run without a device
// (the CPU tests, the sanitizer build) and about L1 * L2 / 2 positions per pair, hence the plain loop over a [same][Q1][Q2] table of log p.
// The table's entries are LogP.h's, as the scoring path's own table's are (hc_api.cpp: build_lut).  tests/golden/self_overlap.json (the
// reference's function run whole) pins the mirror, and tests/test_gpu_self_overlap.py compares the device's scores with the oracle's
// overlap_score bit for bit, independently of the mirror.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/hcsr.h"
#include "LogP.h"
#include "SrConsensus.h"
#include "SrSelfCheck.h"

namespace hc {
namespace srself {

constexpr uint32_t kQ = 94;  // quality bytes 33 .. 126 as Q = byte - 33

struct Tables {
    std::vector<double> lp;  // [same][Q1][Q2]
    double t_same[sr::kQDim], t_other[sr::kQDim];
    uint32_t min_read_len;
    Tables(double mismatch, uint32_t min_read_len_) : lp(2 * kQ * kQ), min_read_len(min_read_len_) {
        for (uint32_t m = 0; m < 2; m++)
            for (uint32_t a = 0; a < kQ; a++)
                for (uint32_t b = 0; b < kQ; b++) lp[(m * kQ + a) * kQ + b] = log_p((int)a, (int)b, m == 1, mismatch);
        for (uint32_t q = 0; q < sr::kQDim; q++) sr::terms((int)q, t_same[q], t_other[q]);
    }
};

struct Mates {
    const uint8_t *b1, *q1, *b2, *q2;
    uint32_t len1, len2;
};

// HC_SR_SELF_BAD_PAIR / HC_SR_SELF_BAD_SYMBOL, or HC_SR_SELF_NONE for a pair the scan may read (hcsr.h)
inline uint32_t check_pair(const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes, const hc_sr_pair& P) {
    if (!pair_in_range(n_bytes, P)) return HC_SR_SELF_BAD_PAIR;  // (SrSelfCheck.h: shared with the device's check)
    for (int mate = 0; mate < 2; mate++) {
        const uint64_t off = mate ? P.off2 : P.off1;
        const uint32_t len = mate ? P.len2 : P.len1;
        for (uint32_t i = 0; i < len; i++)
            if (symbol_bad(seq[off + i], qual[off + i])) return HC_SR_SELF_BAD_SYMBOL;
    }
    return HC_SR_SELF_NONE;
}

// overlap_score (src/EdgeCalculator.cpp:67-139) of a checked pair at offset pos
inline double overlap_score(const Tables& T, const Mates& M, uint32_t pos) {
    if (pos >= M.len1) return 0;                                          // :76-79
    if (M.len1 < T.min_read_len || M.len2 < T.min_read_len) return 0;   // :82-84
    const uint32_t L = std::min(M.len1 - pos, M.len2);
    double total_score = 0.0, total_len = 0.0;
    for (uint32_t i = 0; i < L; i++) {
        const uint8_t n1 = M.b1[i + pos], n2 = M.b2[i];
        if (n1 == 'N' || n2 == 'N') continue;  // score() returns 1, :35-39, :122-124
        const double s = T.lp[((n1 == n2 ? 1u : 0u) * kQ + (uint32_t)(M.q1[i + pos] - 33)) * kQ + (uint32_t)(M.q2[i] - 33)];
        if (!(s <= 0)) return 0;  // :125-127
        total_score += s;
        total_len += 1;
    }
    if (total_len == 0) return 0;
    total_score = (1.0 / total_len) * total_score;  // :137
    return exp(total_score);
}

// consensus() as merge_self_overlap calls it (:890-903): members {mate 1 at 0, mate 2 at p}, total_len = len2 + p, no error correction.
// false: consensus_pos returned 0 somewhere and the strings came back empty.
inline bool merge_at(const Tables& T, const Mates& M, uint32_t p, double min_qual, std::vector<uint8_t>& seq, std::vector<uint8_t>& qual) {
    const uint32_t total_len = M.len2 + p;
    seq.clear();
    qual.clear();
    for (uint32_t c = 0; c < total_len; c++) {
        sr::Sums sums;
        uint32_t k = 0;
        if (c < M.len1) {
            sums.add(code_of(M.b1[c]), T.t_same[M.q1[c] - 33], T.t_other[M.q1[c] - 33]);
            k++;
        }
        if (c >= p) {
            sums.add(code_of(M.b2[c - p]), T.t_same[M.q2[c - p] - 33], T.t_other[M.q2[c - p] - 33]);
            k++;
        }
        uint8_t o[2];
        if (!sr::finish(sums.s[0], sums.s[1], sums.s[2], sums.s[3], k, min_qual, o)) {
            seq.clear();
            qual.clear();
            return false;
        }
        seq.push_back(o[0]);
        qual.push_back(o[1]);
    }
    return true;
}

// (first_offset, the first offset the scan tries, :879-882: SrSelfCheck.h)

// the scan of :879-953 from offset `from` downwards.  Returns the offset taken (seq / qual hold the merged read, *score its score) or -1.
inline int32_t scan_pair(const Tables& T, const Mates& M, uint32_t from, const hc_sr_self_settings& st, double* score, std::vector<uint8_t>& seq,
                         std::vector<uint8_t>& qual) {
    for (uint32_t p = from; p >= 1; p--) {
        const double s = overlap_score(T, M, p);
        if (s > st.min_score && merge_at(T, M, p, st.min_qual, seq, qual)) {
            *score = s;
            return (int32_t)p;
        }
    }
    seq.clear();
    qual.clear();
    *score = 0;
    return -1;
}

}  // namespace srself
}  // namespace hc
