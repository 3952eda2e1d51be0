// hc_sr_self.h — what the self-overlap kernels (hc_sr_self_kernels.hip) and their glue (hc_api_sr.cpp) share.
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

// lut: the 16-bit-symbol layout of hc_device.h (two triangles); qmap: quality byte -> row; inv_n[k] = 1.0 / k; skip[i] != 0: pair i is not scanned
hipError_t sr_self_launch_scan(uint32_t n_cu, uint32_t lanes, const uint8_t* seq, const uint8_t* qual, const hc_sr_pair* pairs, const uint32_t* skip,
                               uint64_t n_pairs, const uint8_t* qmap, const double* lut, const double* inv_n, const SrSelfParams& prm, SrSelfScan* out,
                               hipStream_t s);
// one lane per output column: pair i owns columns [off[i], off[i + 1]); mpos[i] = its offset, < 0: the columns are not the device's
hipError_t sr_self_launch_merge(const uint8_t* seq, const uint8_t* qual, const hc_sr_pair* pairs, uint64_t n_pairs, const int32_t* mpos,
                                const uint64_t* off, uint64_t total, const double* terms, const uint8_t* table, uint8_t* out_seq, uint8_t* out_qual,
                                hipStream_t s);

}  // namespace hc
