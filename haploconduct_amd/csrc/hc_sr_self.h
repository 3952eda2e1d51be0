// hc_sr_self.h — what the self-overlap kernels (hc_sr_self_kernels.hip) and their glue (hc_api_sr.cpp) share.  The tests of a pair that host
// and device share are in host/SrSelfCheck.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcsr.h"
#include "hc_device.h"

namespace hc {

constexpr uint32_t kSelfCap = 2048;     // symbols of each mate the scan keeps in LDS; longer mates go through in windows
constexpr uint32_t kSelfWindow = 1024;  // positions of one window (kSelfWindow + the chunk's offsets - 1 <= kSelfCap symbols of mate 1)
constexpr uint32_t kSelfMaxChunk = 256; // offsets of one chunk = lanes of the workgroup (64, 128, 192 or 256)
constexpr uint32_t kSelfLdsLutBytes = 48u << 10;  // a log table up to this size sits in LDS beside the mates, a larger one stays in device memory
static_assert(kSelfWindow + kSelfMaxChunk - 1 <= kSelfCap, "a window of mate 1 fits the LDS buffer");

constexpr uint32_t kSelfNone = 0, kSelfHit = 1, kSelfBand = 2;
struct SrSelfScan {  // what the scan found for one pair
    int32_t p;       // the largest offset that is a hit or lies in the guard band; -1: none
    uint32_t kind;   // kSelf*
    double x;        // (1.0 / n) * sum of log p at p; -inf where overlap_score returns 0
};
static_assert(sizeof(SrSelfScan) == 16, "SrSelfScan is 16 bytes");

struct SrSelfParams {
    Band band;              // x-space image of min_score
    uint32_t always;        // min_score < 0: every offset passes
    uint32_t min_overlap;
    uint32_t min_read_len;
    uint32_t K;             // quality values of the batch; the log table has K + 2 rows (row K: N)
    uint32_t lut_doubles;
    uint32_t inv_len;       // entries of inv_n
};

// What sr_self_check_kernel leaves of a batch beside the pairs' statuses (hc_sr_merge_self_overlaps_kept): over the VALID pairs, as the
// host-input call's own loop collects them.  Zeroed by the caller before the launch.
struct SrSelfCheckCounters {
    uint32_t qmask[4];   // bit q: quality byte q occurs in a valid pair
    uint32_t max_len;    // max(len1, len2)
    uint32_t max_first;  // the largest first offset (host/SrSelfCheck.h: first_offset)
    uint64_t sum_first;  // the sum of the first offsets: hc_sr_self_stats::n_offsets
    uint64_t n_valid;
};
static_assert(sizeof(SrSelfCheckCounters) == 40, "SrSelfCheckCounters is 40 bytes");
constexpr uint32_t kSelfPad = 16;  // bytes the check kernel's 16-byte loads may touch behind the last mate: the buffers hold as many more

// One copy of sr_self_copy_kernel: src[src1, src1 + len1) and src[src2, src2 + len2) go to dst[dst, dst + len1 + len2), bases and qualities
// alike.  Gathers the mates of a host-decided pair into the staging block, and writes a host-decided pair's merged read behind the kept bytes.
struct SrSelfSeg {
    uint64_t src1, src2, dst;
    uint32_t len1, len2;
};
static_assert(sizeof(SrSelfSeg) == 32, "SrSelfSeg is 32 bytes");

// status[i] = HC_SR_SELF_NONE / _BAD_PAIR / _BAD_SYMBOL of pair i against n_bytes of seq / qual, which must be 16-byte aligned and hold
// kSelfPad bytes behind n_bytes; *counters: see above
hipError_t sr_self_launch_check(const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes, const hc_sr_pair* pairs, uint64_t n_pairs,
                                uint32_t min_overlap, uint32_t* status, SrSelfCheckCounters* counters, hipStream_t s);
// one wave per segment record, 16 bytes a lane and step
hipError_t sr_self_launch_copy(const SrSelfSeg* segs, uint64_t n, const uint8_t* src_seq, const uint8_t* src_qual, uint8_t* dst_seq,
                               uint8_t* dst_qual, hipStream_t s);
// lut: the 16-bit-symbol layout of hc_device.h (two triangles); qmap: quality byte -> row; inv_n[k] = 1.0 / k; skip[i] != 0: pair i is not scanned
hipError_t sr_self_launch_scan(uint32_t n_cu, uint32_t lanes, const uint8_t* seq, const uint8_t* qual, const hc_sr_pair* pairs, const uint32_t* skip,
                               uint64_t n_pairs, const uint8_t* qmap, const double* lut, const double* inv_n, const SrSelfParams& prm, SrSelfScan* out,
                               hipStream_t s);
// one lane per output column: pair i owns columns [off[i], off[i + 1]); mpos[i] = its offset, < 0: the columns are not the device's
hipError_t sr_self_launch_merge(const uint8_t* seq, const uint8_t* qual, const hc_sr_pair* pairs, uint64_t n_pairs, const int32_t* mpos,
                                const uint64_t* off, uint64_t total, const double* terms, const uint8_t* table, uint8_t* out_seq, uint8_t* out_qual,
                                hipStream_t s);

}  // namespace hc
