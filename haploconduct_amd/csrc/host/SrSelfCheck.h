// SrSelfCheck.h — the tests of one pair of hc_sr_merge_self_overlaps / hc_sr_merge_self_overlaps_kept (include/hcsr.h) that read no
// libm: whether the pair's mates lie inside the buffers (HC_SR_SELF_BAD_PAIR) and whether a symbol is one the scan may read
// (HC_SR_SELF_BAD_SYMBOL).  For host and device: check_pair (host/SrSelfOverlap.h) and sr_self_check_kernel (hc_sr_self_kernels.hip)
// take both from here, so that the two cannot drift.  Plain C++ that also compiles as device code.
#pragma once
#include <stdint.h>

#include "../../../include/hcsr.h"
#include "SrCodes.h"

namespace hc {
namespace srself {

// false: HC_SR_SELF_BAD_PAIR — an empty mate (the asserts of src/EdgeCalculator.cpp:70-73), len1 + len2 beyond int32_t, or a mate that
// does not lie inside n_bytes.  Reads the pair alone, no base or quality byte.
HC_SR_HD inline bool pair_in_range(uint64_t n_bytes, const hc_sr_pair& P) {
    if (P.len1 == 0 || P.len2 == 0 || (uint64_t)P.len1 + P.len2 > (uint64_t)INT32_MAX) return false;
    if (P.off1 > n_bytes || P.len1 > n_bytes - P.off1 || P.off2 > n_bytes || P.len2 > n_bytes - P.off2) return false;
    return true;
}

// a base outside ACGTN or a quality byte outside [33,126] (the reference asserts on one, src/EdgeCalculator.cpp:29-30,61)
HC_SR_HD inline bool symbol_bad(uint8_t base, uint8_t q) { return code_of(base) > kCodeN || q < 33 || q > 126; }

// The same test on four symbols at once, for the device's 16-byte loads (and, on the host, for the test that holds it against symbol_bad).
// 0x80 in every byte of w that equals the byte c, exactly (no carry crosses a byte)
HC_SR_HD inline uint32_t bytes_equal(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}
// 0x80 in every byte of (bases, quals) whose symbol symbol_bad refuses
HC_SR_HD inline uint32_t bytes_bad(uint32_t b, uint32_t q) {
    const uint32_t base_ok = bytes_equal(b, 'A') | bytes_equal(b, 'C') | bytes_equal(b, 'G') | bytes_equal(b, 'T') | bytes_equal(b, 'N');
    const uint32_t q7 = q & 0x7F7F7F7Fu;
    // per byte: bit 7 of q7 + 95 is set where q7 >= 33, bit 7 of q7 + 1 where q7 == 127; q itself has it where q >= 128
    const uint32_t q_bad = ~(q7 + 0x5F5F5F5Fu) | (q7 + 0x01010101u) | q;
    return (~base_ok | q_bad) & 0x80808080u;
}
// 0x80 in the bytes [lo, hi) of a word, lo and hi clamped to [0, 4]: the bytes of a load that lie inside a mate
HC_SR_HD inline uint32_t bytes_between(int64_t lo, int64_t hi) {
    if (lo < 0) lo = 0;
    if (hi > 4) hi = 4;
    if (hi <= lo) return 0u;
    const uint32_t below_hi = hi == 4 ? 0xFFFFFFFFu : (1u << (8 * (uint32_t)hi)) - 1u;
    const uint32_t below_lo = (1u << (8 * (uint32_t)lo)) - 1u;  // (lo <= 3)
    return below_hi & ~below_lo & 0x80808080u;
}

// the first offset the scan tries (:879-882), 0 = none
HC_SR_HD inline uint32_t first_offset(uint32_t len1, uint32_t min_overlap) { return len1 > min_overlap ? len1 - min_overlap : 0u; }

}  // namespace srself
}  // namespace hc
