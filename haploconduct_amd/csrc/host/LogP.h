// LogP.h — what EdgeCalculator::score returns for two called bases (reference src/EdgeCalculator.cpp:40-55), with the host's libm: the
// entries of the scoring path's log table (hc_api.cpp: build_lut) and of the self-overlap mirror's (SrSelfOverlap.h).  Own text; the
// expression is the reference's, operation for operation, because every score depends on how libm rounds it.
#pragma once
#include <cmath>
#include <limits>

namespace hc {

// log(p) for the qualities Q1, Q2 and bases that agree (`same`) or differ, or +inf where score() returns 2 ("p < program_settings.mismatch")
inline double log_p(int Q1, int Q2, bool same, double mismatch) {
    const double p1 = pow(10, -Q1 / 10.0);  // phred_to_prob, :59-63
    const double p2 = pow(10, -Q2 / 10.0);
    const double p = same ? (1 - p1) * (1 - p2) + (p1 * p2) / 3.0                                // :41
                          : p1 * (1 - p2) / 3.0 + p2 * (1 - p1) / 3.0 + (2 / 9.0) * p1 * p2;  // :44
    return p < mismatch ? std::numeric_limits<double>::infinity() : log(p);                  // :49-52
}

}  // namespace hc
