// SrConsensus.h — the arithmetic of SRBuilder::consensus_pos (reference src/SRBuilder.cpp:289-409) with the host's libm, shared by the
// host mirror (SrConsensus.cpp) and the device call's glue (hc_api_sr.cpp): the per-quality terms the device adds, the finish of a
// column from its four sums, and the table of one- and two-member columns.  Own text; the expressions are the reference's, operation
// for operation, because every result byte depends on how libm rounds them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/hcsr.h"
#include "SrCodes.h"  // the base codes, the table's geometry and entry codes, kSafeLead / kSafeFloor

namespace hc {
int set_last_error(int status, const std::string& what);  // hc_api.cpp (or the sanitizer build's stub)
namespace sr {

// log10(1 - p) and log10(p / 3.0) with p = phred_to_prob(Q) = pow(10, -Q/10.0)   (:289-293, :316-344)
inline void terms(int Q, double& t_same, double& t_other) {
    const double p = pow(10, -Q / 10.0);
    t_same = log10(1 - p);
    t_other = log10(p / 3.0);
}

// :348-408 from the four sums of a column of n members (N members included in n, :362).  out[0] = nucleotide, out[1] = quality byte.
// Returns 1, or 0 where consensus_pos returns 0 ("p_incorrect NaN", :367-370).
inline int finish(double score_A, double score_C, double score_G, double score_T, uint32_t n, double min_qual, uint8_t* out) {
    const double max_score = std::max({score_A, score_T, score_C, score_G});
    const double max_prob = std::pow(10.0, max_score);
    const double total_prob = std::pow(10.0, score_A) + std::pow(10.0, score_T) + std::pow(10.0, score_C) + std::pow(10.0, score_G);
    if (max_score == 0 || total_prob == 0.0) {
        out[0] = 'N';
        out[1] = '$';
        return 1;
    }
    const double p_incorrect = 1 - (max_prob / total_prob);
    if (n > 1 && (1 - p_incorrect) < min_qual) {
        out[0] = 'N';
        out[1] = '$';
        return 1;
    }
    if (p_incorrect != p_incorrect) return 0;
    int phred;
    if (p_incorrect < std::pow(10.0, -9.3)) phred = 93;
    else phred = (int)round(-10 * log10(p_incorrect));
    if (phred < 0) phred = 0;
    else if (phred > 93) phred = 93;
    uint8_t nuc;  // tie order A, T, C, G (:390-393)
    if (max_score == score_A) nuc = 'A';
    else if (max_score == score_T) nuc = 'T';
    else if (max_score == score_C) nuc = 'C';
    else nuc = 'G';  // (max_score is one of the four unless a sum is NaN, which the branch above has taken)
    out[0] = nuc;
    out[1] = (uint8_t)(phred + 33);
    return 1;
}

// the sums of :299-346: every member adds its term to all four scores, in list order
struct Sums {
    double s[4] = {0, 0, 0, 0};  // by base code A, C, G, T
    inline void add(uint32_t code, double t_same, double t_other) {
        if (code > 3) return;  // 'N': counted in the column's length only
        for (uint32_t x = 0; x < 4; x++) s[x] += (x == code) ? t_same : t_other;
    }
};

inline uint8_t entry_of(const Sums& u, uint32_t n, double min_qual) {
    uint8_t o[2];
    if (!finish(u.s[0], u.s[1], u.s[2], u.s[3], n, min_qual, o)) return kEntryNaN;
    return o[0] == 'N' ? kEntryN : (uint8_t)(o[1] - 33);
}

// The table of hcsr.h (hc_host_sr_table) for the quality values `qs` (q = byte - 33).  The total of the four probabilities is added in
// the order A, T, C, G (:350), so an entry depends on WHICH bases the members have, not only on whether they agree: the table is
// indexed by both base codes.
inline void build_table(double min_qual, const std::vector<uint32_t>& qs, uint8_t* table) {
    memset(table, kEntryN, HC_SR_TABLE_BYTES);
    std::vector<double> ts(kQDim, 0.0), to(kQDim, 0.0);
    for (uint32_t q : qs) terms((int)q, ts[q], to[q]);
    const std::vector<uint32_t> qn{0};  // an N member's quality takes no part: its entries sit at q = 0
    for (uint32_t b1 = 0; b1 < 5; b1++) {
        for (uint32_t q1 : (b1 == 4 ? std::vector<uint32_t>{0} : qs)) {
            Sums u1;
            u1.add(b1, ts[q1], to[q1]);
            const uint8_t e1 = entry_of(u1, 1, min_qual);
            for (uint32_t qa : (b1 == 4 ? qn : std::vector<uint32_t>{q1})) table[kTable1 + b1 * kQDim + qa] = e1;
            for (uint32_t b2 = 0; b2 < 5; b2++) {
                for (uint32_t q2 : (b2 == 4 ? std::vector<uint32_t>{0} : qs)) {
                    Sums u2 = u1;
                    u2.add(b2, ts[q2], to[q2]);
                    const uint8_t e2 = entry_of(u2, 2, min_qual);
                    for (uint32_t qa : (b1 == 4 ? qn : std::vector<uint32_t>{q1}))
                        for (uint32_t qb : (b2 == 4 ? qn : std::vector<uint32_t>{q2}))
                            table[((b1 * 5 + b2) * kQDim + qa) * kQDim + qb] = e2;
                }
            }
        }
    }
}

// Whether the device may finish a deeper column itself (SrCodes.h: kSafeLead, kSafeFloor) — then Phred 93 and the minQual test pass
// whatever libm rounds.
inline bool safe_region_allowed(double min_qual) { return min_qual <= 1 - 1e-9; }

// The packed output buffers a, b of `cap` bytes are to take `total` bytes: HC_OK, or the error of entry point `fn`, whose argument
// `counter` has been given the size to come back with.
inline int check_room(const char* fn, const char* buffers, const char* counter, uint64_t total, uint64_t cap, const void* a, const void* b) {
    if (total <= cap && (total == 0 || (a && b))) return HC_OK;
    return set_last_error(HC_ERR_ARG, std::string(fn) + ": " + buffers + " have no room (*" + counter + " says how much is needed)");
}

}  // namespace sr
}  // namespace hc
