// hc_fno3_walk.h — what hc_fno3_from_originals (include/hcsr.h) shares between its kernels (hc_fno3_walk_kernels.hip), its glue
// (hc_api_fno3_resident.cpp) and the host mirror (host/FindNextOverlaps.cpp): the walk rank of a read, the differences deduceOverlap reads
// an original through, and the argument checks.  Plain C++ without hipcc, as hc_fno_items.h: the mirror builds without HIP.  Internal: not
// part of the ABI.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/hcsr.h"
#include "hc_fno_items.h"

namespace hc {
namespace fno3w {

constexpr uint64_t kMaxCombos = (1ull << 31) - 16;

// the place of read r in single_SR_vec ++ paired_SR_vec ++ trivial_SR_vec when ids run singles, trivials, pairs
struct Ranks {
    const uint32_t* walk_rank;  // NULL: from the counts
    uint64_t n_single, n_trivial, n_paired;
};
HC_FNO_HD inline uint32_t rank_of(const Ranks& k, uint64_t r) {
    if (k.walk_rank) return k.walk_rank[r];
    if (r < k.n_single) return (uint32_t)r;
    if (r < k.n_single + k.n_trivial) return (uint32_t)(r + k.n_paired);
    return (uint32_t)(r - k.n_trivial);
}

// (d_l, d_r) of one shared original: what deduceOverlap reads of it, in the reference's int arithmetic
struct Diff {
    int32_t l, r;
};
HC_FNO_HD inline Diff diff_of(const hc_sr_original& a, const hc_sr_original& b, bool either_paired) {
    return Diff{(int32_t)((uint32_t)a.index1 - (uint32_t)b.index1), either_paired ? (int32_t)((uint32_t)a.index2 - (uint32_t)b.index2) : 0};
}

HC_FNO_HD inline int bits_for(uint64_t n) {  // bits that hold every value below n (at least 1)
    int b = 1;
    while (b < 63 && (1ull << b) < n) b++;
    return b;
}

// the record fno3_deduce takes (hc_fno_items.h, kind 4)
HC_FNO_HD inline FnoItem item_of(uint64_t ida, uint64_t idb, const hc_sr_original& ea, const hc_sr_original& eb, uint32_t a_len1,
                                           uint32_t a_len2, bool a_paired, uint32_t b_len1, uint32_t b_len2, bool b_paired) {
    FnoItem it{};
    it.ida = ida;
    it.idb = idb;
    it.v[0] = ea.index1;
    it.v[1] = ea.index2;
    it.v[2] = eb.index1;
    it.v[3] = eb.index2;
    it.v[4] = (int32_t)a_len1;
    it.v[5] = a_paired ? (int32_t)a_len2 : 0;
    it.v[6] = (int32_t)b_len1;
    it.v[7] = b_paired ? (int32_t)b_len2 : 0;
    it.kind = 4;
    it.a_paired = a_paired;
    it.b_paired = b_paired;
    return it;
}

// host/FindNextOverlaps.cpp: nullptr, or what is wrong with the arguments (HC_ERR_ARG)
const char* check_input(const hc_fno3_resident_input* in, uint64_t n_reads);

#if defined(__HIPCC__)
// device side.  Every array is the caller's; n_* below 2^31.
struct Dict {
    const uint64_t* off;
    const hc_sr_original* entries;
    uint64_t n_reads, n_entries;
};
struct Work {
    // per entry
    uint64_t* key1_in;     // original id << 32 | walk rank
    uint64_t* key1;        // sorted
    uint32_t* val1_in;     // the entry
    uint32_t* val1;        // sorted
    uint32_t* entry_read;  // the read that owns entry e
    uint8_t* head1;        // sorted place p starts a run of one original
    uint32_t* head1_pos;   // the heads' places
    uint64_t* cnt;         // n_entries + 1: combinations the entry at sorted place p owns, then their exclusive sum in place
    // per combination
    uint64_t* key2_in;     // rank of SR1 << b | rank of SR2
    uint64_t* key2;
    uint32_t* val2_in;     // the combination
    uint32_t* val2;
    Diff* diff;            // per combination, unsorted
    uint8_t* head2;        // sorted place u starts a run of one pair
    uint32_t* differs;     // n_combos + 1: u differs from u - 1 inside a run, then the exclusive sum in place
    uint32_t* head2_pos;   // the candidates' places
    // counters[0] largest original id, [1] originals, [2] candidates, [3] ambiguous candidates; from kDeduceCounters on: fno3_deduce's
    unsigned long long* counters;
};
constexpr int kDeduceCounters = 8, kCounters = 16;
hipError_t launch_keys1(Dict D, Ranks K, Work W, hipStream_t s);
hipError_t launch_heads1(Work W, uint64_t n_entries, hipStream_t s);
hipError_t launch_count(Work W, uint64_t n_entries, hipStream_t s);  // reads counters[1]
hipError_t launch_combos(Dict D, const void* descs, Work W, uint64_t n_combos, int rank_bits, hipStream_t s);
hipError_t launch_heads2(Work W, uint64_t n_combos, hipStream_t s);
hipError_t launch_items(Dict D, const void* descs, Work W, uint64_t n_combos, uint64_t n_cand, FnoItem* items, hc_fno3_candidate* cands, hipStream_t s);
hipError_t launch_line_flags(const uint64_t* len, uint64_t n_cand, hc_fno3_candidate* cands, hipStream_t s);
#endif

}  // namespace fno3w
}  // namespace hc
