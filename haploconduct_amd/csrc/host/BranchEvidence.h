// BranchEvidence.h — what hc_br_evidence (include/hcsr.h) and its host mirror share: the expressions of the reference's
// buildDiffListOut / buildDiffListIn / checkReadEvidence (src/BranchReduction.cpp:396-743) that depend on integer widths, written once
// for the kernels (hc_br_kernels.hip) and for host/BranchEvidence.cpp.  Plain C++: the host file also builds without HIP.
#pragma once
#include <stdint.h>

#include <string>

#include "../../../include/hcsr.h"

#if defined(__HIPCC__)
#define HC_BR_HD __host__ __device__
#else
#define HC_BR_HD
#endif

namespace hc {
int set_last_error(int status, const std::string& what);  // (hc_scratch.h)

namespace br {

// build_rev_comp (src/Types.h:109-129); a byte it exits on stays as it is (hc_sr_next.h: sr_next_complement is the same table)
HC_BR_HD inline uint8_t complement(uint8_t b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b; }

// base k of a stored sequence (len bytes at s) in the orientation fwd: get_seq(0) or get_rev_comp(0)
HC_BR_HD inline uint8_t oriented(const uint8_t* s, uint64_t len, bool fwd, uint64_t k) { return fwd ? s[k] : complement(s[len - 1 - k]); }

// int(seq.size() - program_settings.min_overlap_len), :449: a size_t difference cut to 32 bits
HC_BR_HD inline int32_t size_minus_min_overlap(uint64_t size, uint32_t min_overlap_len) { return (int32_t)(uint32_t)(size - (uint64_t)min_overlap_len); }

// (int)floor(100 * len / std::min(seq_i.size(), seq_j.size())), :487: an int product divided as size_t
HC_BR_HD inline int32_t overlap_perc(int32_t len, uint64_t min_size) {
    const uint64_t num = (uint64_t)(int64_t)(int32_t)(100u * (uint32_t)len);
    return (int32_t)(num / min_size);
}

// int x = a + b where a is an int and b a size_t (:720, :722): the 64-bit sum cut to 32 bits
HC_BR_HD inline int32_t int_plus_size(int32_t a, uint64_t b) { return (int32_t)(uint32_t)((uint64_t)(int64_t)a + b); }

// int dist = 0.5 * (min + max), :523: toward zero, which is what the integer division does
HC_BR_HD inline int32_t half_toward_zero(int32_t mn, int32_t mx) { return (int32_t)((uint32_t)mn + (uint32_t)mx) / 2; }

// the mate of an original id (:270-284): false for a single-end original
HC_BR_HD inline bool mate_of(uint64_t id, uint64_t se, uint64_t pe, uint64_t* mate) {
    if (id >= se + pe) return *mate = id - pe, true;
    if (id >= se) return *mate = id + pe, true;
    return false;
}

// argument checks the device call and the mirror share; nullptr: fine
const char* check_settings(const hc_br_settings* st, uint64_t n_original_reads);
const char* check_original_reads(const uint8_t* bases, const uint64_t* seq_off, uint64_t n_reads);

}  // namespace br
}  // namespace hc
