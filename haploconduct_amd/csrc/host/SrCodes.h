// SrCodes.h — the base codes of the store and the geometry of the consensus tables (include/hcsr.h: hc_host_sr_table), for host and device:
// the kernels (hc_kernels.hip, hc_sr_kernels.hip, hc_sr_self_kernels.hip), their glue and the host mirrors read them here and nowhere else.
// Plain C++ that also compiles as device code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HC_SR_HD __host__ __device__
#else
#define HC_SR_HD
#endif

namespace hc {

constexpr uint32_t kCodeN = 4;
constexpr uint32_t kCodeBadQual = 6;  // (a store symbol's: hc_device.h)
constexpr uint32_t kCodeBadBase = 7;

// base code of a byte: A, C, G, T = 0..3, N, anything else kCodeBadBase; the complement of a code < 4 is 3 - code
HC_SR_HD inline uint32_t code_of(uint8_t c) {
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? kCodeN : kCodeBadBase;
}
// the same for a symbol that was checked before: whatever is not ACGT is N
HC_SR_HD inline uint32_t code_or_n(uint8_t c) {
    const uint32_t code = code_of(c);
    return code == kCodeBadBase ? kCodeN : code;
}

namespace sr {

constexpr uint32_t kQDim = 128;                    // quality bytes 33 .. 127 as q = byte - 33 < 128; the term tables have as many entries
constexpr uint32_t kTable1 = 25u * kQDim * kQDim;  // where the one-member entries of the table start
constexpr uint8_t kEntryN = 255, kEntryNaN = 254;  // 'N' / '$' column; consensus_pos returns 0
// A column of three or more members that the device may finish itself (DESIGN.md "Super-read consensus"): the largest sum leads every
// other by at least 9.3 + log10(3) + 0.01 decades, lies in (-300, 0), and min_qual <= 1 - 1e-9 (SrConsensus.h: safe_region_allowed).
constexpr double kSafeLead = 9.79;  // > 9.3 + log10(3) + 0.01 = 9.7871...
constexpr double kSafeFloor = -300.0;

}  // namespace sr
}  // namespace hc
