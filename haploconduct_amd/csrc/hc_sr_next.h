// hc_sr_next.h — what the device kernels (hc_sr_next_kernels.hip), the glue (hc_api_sr_next.cpp) and the host mirror
// (host/SrNextReads.cpp) of hc_sr_set_next_reads (include/hcsr.h) share: how an entry resolves to its mates, the tests in the
// reference's order, build_rev_comp's mapping, and the launch interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcsr.h"

namespace hc {

// where a mate's bytes lie: the kept consensus bytes, the call's extra bytes, the raw arrays of the current store
constexpr uint32_t kNextSrcRaw = 2;
constexpr uint32_t kNextMaxLen = 1u << 28;  // hc_set_reads refuses a sequence of 2^28 bases and more

struct SrNextMate {
    uint64_t off;
    uint32_t len, src;
};
// the mates of an entry in OUTPUT order (a reverse pair has its mates swapped, :1342), n_mates of them
struct SrNextResolved {
    SrNextMate m[2];
    uint32_t n_mates, rev;
};
struct SrNextSources {
    uint64_t n_cons, n_extra;     // bytes of the two packed sources
    const uint64_t* raw_off;      // the current store: seq_off (n_seq + 1) and read_first_seq (n_reads + 1)
    const uint32_t* raw_first;
    uint32_t n_reads;
};

// false: HC_SR_NEXT_BAD_ENTRY.  Reads the entry and, for a trivial, the store's offsets — no base or quality byte.
__host__ __device__ inline bool sr_next_resolve(const hc_sr_next_entry& e, const SrNextSources& S, SrNextResolved& R) {
    R.n_mates = 0;
    R.rev = 0;
    if (e.kind > HC_SR_NEXT_TRIVIAL_PAIRED || e.rev > 1) return false;
    if (e.kind == HC_SR_NEXT_SINGLE || e.kind == HC_SR_NEXT_PAIRED) {
        const uint32_t nm = e.kind == HC_SR_NEXT_PAIRED ? 2u : 1u;
        for (uint32_t k = 0; k < nm; k++) {
            const uint32_t src = k ? e.src2 : e.src1, len = k ? e.len2 : e.len1;
            const uint64_t off = k ? e.off2 : e.off1;
            if (src > HC_SR_SRC_BYTES || len >= kNextMaxLen) return false;
            const uint64_t room = src == HC_SR_SRC_CONSENSUS ? S.n_cons : S.n_extra;
            if (off > room || len > room - off) return false;
            R.m[k] = SrNextMate{off, len, src};
        }
        R.n_mates = nm;
        return true;
    }
    if (e.read >= S.n_reads) return false;
    const uint32_t q = S.raw_first[e.read], nm = S.raw_first[e.read + 1] - q;
    if (nm != (e.kind == HC_SR_NEXT_TRIVIAL_PAIRED ? 2u : 1u)) return false;
    for (uint32_t k = 0; k < nm; k++) {
        const uint32_t s = q + ((e.rev && nm == 2) ? 1u - k : k);  // (rev_comp(2), rev_comp(1))
        R.m[k] = SrNextMate{S.raw_off[s], (uint32_t)(S.raw_off[s + 1] - S.raw_off[s]), kNextSrcRaw};
    }
    R.n_mates = nm;
    R.rev = e.rev;
    return true;
}

// Read::test_N_rate (src/Read.h:226-232): one IEEE multiply and one compare in fp64; the library is built without contraction
__host__ __device__ inline bool sr_next_n_rate_ok(uint64_t n_count, uint64_t len) { return (double)n_count < 0.05 * (double)len; }

// the tests of a resolved entry, given the N count of its mates together
__host__ __device__ inline uint32_t sr_next_status(uint32_t kind, const SrNextResolved& R, uint64_t n_count, uint32_t keep_singletons) {
    uint64_t len = 0;
    for (uint32_t k = 0; k < R.n_mates; k++) len += R.m[k].len;
    if (kind <= HC_SR_NEXT_PAIRED) {
        for (uint32_t k = 0; k < R.n_mates; k++)
            if (R.m[k].len == 0) return HC_SR_NEXT_DROPPED_EMPTY;  // :983, :999
    } else if (len < keep_singletons) {
        return HC_SR_NEXT_DROPPED_SHORT;  // :1286
    }
    return sr_next_n_rate_ok(n_count, len) ? HC_SR_NEXT_KEPT : HC_SR_NEXT_DROPPED_N_RATE;
}

// build_rev_comp (Types.h:109-129); a byte it exits on stays as it is
__host__ __device__ inline uint8_t sr_next_complement(uint8_t b) {
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
}

// (offset, base, quality) of a consensus column the host finished (hc_sr_consensus with keeping on); off = ~0: nothing to write
struct SrPatch {
    uint64_t off;
    uint8_t base, qual, pad[6];
};

// hc_sr_next_kernels.hip.  The packed sources: [0] the kept consensus, [1] the extra bytes, [2] the current raw arrays.
struct SrNextBytes {
    const uint8_t* seq[3];
    const uint8_t* qual[3];
};
// status[i], cnt[i] = kept ? 1 | n_mates << 32 : 0, bytes[i] = kept ? len1 + len2 : 0 (cnt and bytes: n + 1 entries, the last 0)
hipError_t sr_next_launch_check(const hc_sr_next_entry* entries, uint64_t n, SrNextSources S, SrNextBytes B, uint32_t keep_singletons,
                                uint32_t* status, uint64_t* cnt, uint64_t* bytes, hipStream_t stream);
// cnt_off / byte_off: the exclusive sums of cnt / bytes (n + 1 entries).  Writes the survivors' bytes, out_off (n_seq + 1) and out_first
// (n_kept + 1).
hipError_t sr_next_launch_gather(const hc_sr_next_entry* entries, uint64_t n, SrNextSources S, SrNextBytes B, const uint32_t* status,
                                 const uint64_t* cnt_off, const uint64_t* byte_off, uint8_t* out_bases, uint8_t* out_quals, uint64_t* out_off,
                                 uint32_t* out_first, hipStream_t stream);
// hist[0..255] += byte counts of quals, hist[256..511] += of bases (hist zeroed by the caller)
hipError_t sr_next_launch_hist(const uint8_t* bases, const uint8_t* quals, uint64_t total, uint32_t n_cu, unsigned long long* hist,
                               hipStream_t stream);
hipError_t sr_launch_patch(const SrPatch* patches, uint64_t n, uint64_t total, uint8_t* seq, uint8_t* qual, hipStream_t stream);

}  // namespace hc
