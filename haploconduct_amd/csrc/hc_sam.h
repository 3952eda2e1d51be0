// hc_sam.h — launchers of hc_sam_kernels.hip: scripts/sam2overlaps.py's enumeration of (record, active read) pairs in closed form
// (hc_api_sam.cpp drives them; hc_sam_items.h evaluates one pair).  All asynchronous on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"

namespace hc {

enum : unsigned long long {
    kSamStatusScript = 1,  // the count pass met a place where the script dies (an assert, a division by zero)
    kSamStatusRange = 2    // a number hc_line_rec does not hold
};

struct SamSorted {  // the records in the script's order: references in FASTA order, then (position, kind, input order)
    const int32_t* pos;      // key position: the first stored mate's cpos
    const uint32_t* len;     // length of the first stored mate's sequence
    const uint32_t* ref;
    const hc_sam_rec* rec;
    uint32_t n;
};

hipError_t sam_keys(const hc_sam_aln* alns, const hc_sam_rec* recs, uint32_t n, uint64_t* keys, uint32_t* iota, hipStream_t s);
hipError_t sam_gather(const hc_sam_aln* alns, const hc_sam_rec* recs, const uint32_t* perm, uint32_t n, int32_t* pos, uint32_t* len, uint32_t* ref,
                      hc_sam_rec* rec, hipStream_t s);
// proc_end[r] = seg_begin[r] + records of reference r the script's loop processes (:535)
hipError_t sam_processed(const int32_t* pos, const uint32_t* seg_begin, const uint64_t* ref_len, uint32_t n_refs, uint32_t* proc_end, hipStream_t s);
// e[j]: the last i record j is evaluated against (j: none); cand[j] = e[j] - j
hipError_t sam_last_partner(const SamSorted& S, const uint32_t* seg_begin, const uint32_t* proc_end, int64_t mol, uint32_t* e, uint64_t* cand, hipStream_t s);
// m[j] = max(e[0 .. j]); block_max: room for (n + 1023) / 1024 entries
hipError_t sam_prefix_max(const uint32_t* e, uint32_t n, uint32_t* m, uint32_t* block_max, hipStream_t s);
// lo[i]: the lowest j that can still be active when record i is processed (i: nothing to scan); win[i] = i - lo[i]
hipError_t sam_window(const SamSorted& S, const uint32_t* seg_begin, const uint32_t* proc_end, const uint32_t* m, uint32_t* lo, uint64_t* win, hipStream_t s);
// one wave per record i: cnt[i] = lines of record i
hipError_t sam_count(const SamSorted& S, const hc_sam_aln* alns, const hc_sam_op* ops, const uint32_t* lo, const uint32_t* e, int64_t mol, uint64_t* cnt,
                     unsigned long long* status, hipStream_t s);
// range[0], range[1]: first and one past the last record that owns a line of [first_line, first_line + n_lines)
hipError_t sam_owner_range(const uint64_t* off, uint32_t n, uint64_t first_line, uint64_t n_lines, uint32_t* range, hipStream_t s);
// one wave per record of [i0, i1): its lines that fall into [first_line, first_line + n_lines) go to out[line - first_line]
hipError_t sam_write(const SamSorted& S, const hc_sam_aln* alns, const hc_sam_op* ops, const uint32_t* lo, const uint32_t* e, const uint64_t* off, int64_t mol,
                     uint32_t i0, uint32_t i1, uint64_t first_line, uint64_t n_lines, hc_line_rec* out, hipStream_t s);

}  // namespace hc
