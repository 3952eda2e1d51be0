// hc_sr_originals.h — what hc_sr_originals_next (include/hcsr.h) computes per entry, shared by the kernels (hc_sr_originals_kernels.hip),
// the glue (hc_api_sr_originals.cpp) and the host mirror (host/SrOriginals.cpp): the branches of constructSuperread's loop over a
// vertex's originals (reference src/SRBuilder.cpp:766-804), merge_self_overlap's shift (:938-949) and the reversal of a trivial super-read
// (:1193-1214), in 64-bit arithmetic as the reference's long, with the result checked against int32.  Internal: not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcsr.h"

namespace hc {
namespace orig {

constexpr uint32_t kBitEmpty = 1u, kBitSeq0 = 2u, kBitRange = 4u;  // a new read's failures, or-ed; status_of picks the one reported

__host__ __device__ inline uint32_t status_of(uint32_t bits) {
    return bits & kBitEmpty ? HC_SR_ORIG_EMPTY_SOURCE : bits & kBitSeq0 ? HC_SR_ORIG_SEQ0_OF_PAIRED : bits & kBitRange ? HC_SR_ORIG_RANGE : HC_SR_ORIG_OK;
}

// What a source needs of its vertex and, for a super-read's vertex, of its clique.
struct Source {
    int32_t index1, index2, startpos1, startpos2;  // the subread row, index2 as the merge call returned it
    int32_t overlap_pos;                           // >= 0: merge_self_overlap merged the clique
    int32_t len2_layout;                           // the 'r' layout's total_len, 0 without one (:693, :788)
    uint32_t read_len1, read_len2;                 // of the vertex's read
    uint8_t read_paired, fwd, first_it, trivial;
};

__host__ __device__ inline bool fits(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

// e: an entry of the dict of the source's read, changed in place.  Returns the failure bits (0: none).
__host__ __device__ inline uint32_t transform(const Source& s, hc_sr_original& e) {
    int64_t i1 = e.index1, i2 = e.index2;
    const int64_t L1 = s.read_len1, L2 = s.read_len2;
    if (s.trivial) {
        if (!s.fwd) {  // :1193-1199, :1206-1213
            e.forward = !e.forward;
            i1 = L1 - (i1 + (int64_t)e.len1);
            if (e.paired) i2 = (s.read_paired ? L2 : L1) - (i2 + (int64_t)e.len2);
        }
    } else {
        const bool shifted = s.overlap_pos >= 0 && s.index2 >= 0;  // (:918-922 shifts where index2 >= 0, and the sum stays >= 0)
        const int64_t sub2 = shifted ? (int64_t)s.index2 - s.overlap_pos : s.index2;
        const int64_t idx1 = (int64_t)s.index1 - s.startpos1, idx2 = sub2 - s.startpos2;
        e.forward = (e.forward != 0) == (s.fwd != 0);
        if (s.first_it) {
            i1 = idx1;
            if (e.paired) i2 = idx2;
        } else if (s.fwd) {
            i1 += idx1;
            if (e.paired) i2 += sub2 >= 0 ? idx2 : idx1;
        } else if (e.paired) {
            if (s.read_paired) {
                i1 = L1 + idx1 - ((int64_t)e.len1 + i1);
                i2 = L2 + (s.len2_layout > 0 || sub2 >= 0 ? idx2 : idx1) - ((int64_t)e.len2 + i2);
            } else {
                i1 = L1 + idx1 - ((int64_t)e.len1 + i1);
                i2 = L1 + idx1 - ((int64_t)e.len2 + i2);
            }
        } else {
            if (s.read_paired) return kBitSeq0;  // get_seq(0) of a paired read, :801
            i1 = L1 + idx1 - ((int64_t)e.len1 + i1);
        }
        if (s.overlap_pos >= 0 && e.paired) i2 += s.overlap_pos;
    }
    if (!e.paired) i2 = 0, e.len2 = 0;
    if (!fits(i1) || !fits(i2)) return kBitRange;
    e.index1 = (int32_t)i1;
    e.index2 = (int32_t)i2;
    return 0;
}

// The Source of a super-read's vertex.
__host__ __device__ inline Source sr_source(const hc_fno_subread& row, const hc_fno_read& node, uint8_t fwd, uint32_t kind, int32_t overlap_pos,
                                            int32_t len2_layout, uint32_t first_it) {
    return Source{row.index1, row.index2, row.startpos1, row.startpos2, kind == HC_SR_MN_SINGLE_SELF ? overlap_pos : -1, len2_layout,
                  node.len1, node.len2, node.paired, (uint8_t)(fwd != 0), (uint8_t)(first_it != 0), 0};
}
__host__ __device__ inline Source trivial_source(const hc_fno_read& node, uint8_t fwd) {
    return Source{0, 0, 0, 0, -1, 0, node.len1, node.len2, node.paired, (uint8_t)(fwd != 0), 0, 1};
}
__host__ __device__ inline int32_t len2_of(const uint64_t* first_layout, const hc_sr_layout* layouts, uint64_t c) {
    return first_layout[c + 1] - first_layout[c] == 2 ? layouts[first_layout[c] + 1].total_len : 0;
}

// characters of an entry in subreads.txt (:1455-1461): "\tID:+:index1:len1" or "\tID:+:index1,index2:len1,len2"
__host__ __device__ inline uint32_t dec_u32(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10u) v /= 10u, n++;
    return n;
}
__host__ __device__ inline uint32_t dec_i32(int32_t x) { return dec_u32(x < 0 ? 0u - (uint32_t)x : (uint32_t)x) + (x < 0 ? 1u : 0u); }
__host__ __device__ inline uint32_t entry_chars(const hc_sr_original& e) {
    uint32_t n = 1 + dec_u32(e.id) + 3 + dec_i32(e.index1) + 1 + dec_u32(e.len1);
    if (e.paired) n += 1 + dec_i32(e.index2) + 1 + dec_u32(e.len2);
    return n;
}
__host__ __device__ inline char* put_u32(char* p, uint32_t v) {
    const uint32_t n = dec_u32(v);
    for (uint32_t k = n; k-- > 0;) p[k] = (char)('0' + v % 10u), v /= 10u;
    return p + n;
}
__host__ __device__ inline char* put_i32(char* p, int32_t x) {
    if (x < 0) *p++ = '-';
    return put_u32(p, x < 0 ? 0u - (uint32_t)x : (uint32_t)x);
}
__host__ __device__ inline char* put_entry(char* p, const hc_sr_original& e) {
    *p++ = '\t';
    p = put_u32(p, e.id);
    *p++ = ':';
    *p++ = e.forward ? '+' : '-';
    *p++ = ':';
    p = put_i32(p, e.index1);
    if (e.paired) {
        *p++ = ',';
        p = put_i32(p, e.index2);
    }
    *p++ = ':';
    p = put_u32(p, e.len1);
    if (e.paired) {
        *p++ = ',';
        p = put_u32(p, e.len2);
    }
    return p;
}

// host/SrOriginals.cpp: the argument checks the device call and the mirror share.  nullptr: fine; else what is wrong (HC_ERR_ARG).
// *n_cand (check_input) = the candidate entries.
const char* check_dict(const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads);
const char* check_input(const hc_sr_originals_input* in, const hc_sr_originals_output* out, const uint64_t* dict_off, uint64_t dict_reads,
                        uint64_t* n_cand);

// device side (hc_sr_originals_kernels.hip)
struct Dict {
    const uint64_t* off;
    const hc_sr_original* entries;
    uint64_t n_reads, n_entries;
};
struct In {  // hc_sr_originals_input's arrays, on the device
    const uint32_t* kind;
    const int32_t* new_id;
    const int32_t* overlap_pos;
    const uint64_t* first_layout;
    const hc_sr_layout* layouts;
    const uint32_t* sr_clique;
    const uint64_t* subread_off;
    const hc_fno_subread* subreads;
    const uint32_t* vertex_state;
    const hc_fno_read* nodes;
    const uint32_t* vertex_read;
    const uint8_t* vertex_fwd;
    uint64_t n_cliques, n_srs, n_sub, n_vertices, n_new;
    uint32_t first_it;
};
struct Work {
    uint64_t* cnt;       // n_src + 1: candidates per source, then their exclusive sum in cnt_off
    uint64_t* cnt_off;
    uint64_t* key_in;    // per candidate: new id << 32 | original id
    uint64_t* key;
    uint32_t* val_in;    // per candidate: its index
    uint32_t* val;
    hc_sr_original* cand;  // per candidate, transformed; pad[0] = its failure bits
    uint32_t* bits;      // per new read: failure bits
    uint8_t* flag;       // per sorted candidate: kept
    uint32_t* sel;       // the kept ones' sorted positions
    unsigned long long* n_sel;
    uint32_t* out_id;    // per kept entry: its new read
    hc_sr_original* out_entries;
    uint64_t* out_off;   // n_new + 1
    uint32_t* out_status;
};
hipError_t launch_init(const void* descs, uint32_t n_reads, uint64_t* off, hc_sr_original* entries, hipStream_t stream);
hipError_t launch_count(In I, Dict D, Work W, hipStream_t stream);                       // n_src + 1 lanes
hipError_t launch_candidates(In I, Dict D, Work W, uint64_t n_cand, hipStream_t stream);
hipError_t launch_first(Work W, uint64_t n_cand, hipStream_t stream);
hipError_t launch_keep(Work W, uint64_t n_cand, hipStream_t stream);
hipError_t launch_gather(Work W, uint64_t n_cand, hipStream_t stream);
hipError_t launch_offsets(In I, Work W, hipStream_t stream);
hipError_t launch_text_sizes(Dict D, uint64_t* sizes, hipStream_t stream);   // n_entries + n_reads + 1 items
hipError_t launch_text_write(Dict D, const uint64_t* pos, char* text, hipStream_t stream);

}  // namespace orig
}  // namespace hc
