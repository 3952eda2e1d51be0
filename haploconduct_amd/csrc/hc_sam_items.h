// hc_sam_items.h — one (record, active read) of scripts/sam2overlaps.py's get_overlaps (:395-480) as integer arithmetic over the records
// of include/hcedge.h: compute_overlap_pos (:268-313), get_overlap_line's percentage (:333-338), merge_overlaps (:350-369).  The host
// mirror (host/Sam2Overlaps.cpp) and the device's count and write passes (hc_sam_kernels.hip) both evaluate a pair with this text; which
// pairs are evaluated, and in what order, is each side's own (the script's list of active reads there, its closed form here).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hcedge.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HC_SAM_HD __host__ __device__ __forceinline__
#else
#define HC_SAM_HD inline
#endif

namespace hc {

// where the script dies inside a pair (0: it does not)
enum : uint32_t {
    kSamOk = 0,
    kSamAssertCount = 1,  // `assert aln_len > 0`, :298
    kSamAssertPerc = 2,   // `assert perc >= 0` / `assert perc <= 100`, :334, :338
    kSamZeroDivision = 3, // min(len(seq1), len(seq2)) == 0, :333
    kSamRange = 4,        // (not the script's) a number hc_line_rec does not hold
    kSamCigarValue = 5,   // int() of a letter: a CIGAR that starts with one, :276, :280
    kSamCigarIndex = 6    // cigar[i + 1] behind the last count: a CIGAR that ends with one, :276, :279
};

struct SamOverlap {
    int64_t pos, len;
};

// compute_overlap_pos(pos1, pos2, len1, len2, CIGAR1, CIGAR2): read 2 is in front.  Every letter other than D and I consumes both.
HC_SAM_HD SamOverlap sam_overlap_pos(int64_t pos1, int64_t pos2, int64_t len1, int64_t len2, const hc_sam_op* c1, uint32_t n1, const hc_sam_op* c2,
                                     uint32_t n2, uint32_t& err) {
    const int64_t d = pos1 - pos2;
    int64_t back_total = 0;
    for (uint32_t k = 0; k < n1; k++)
        if (c1[k].letter != 'I') back_total += c1[k].count;
    const int64_t max_len = d + back_total;
    int64_t fs = 0, fr = 0, p = 0;
    for (uint32_t k = 0; k < n2; k++) {
        const int64_t len = c2[k].count;
        const uint32_t t = c2[k].letter;
        if (p < max_len) {
            const int64_t take = len < max_len - p ? len : max_len - p;
            if (t != 'D') fs += take;
            if (t != 'I') {
                fr += take;
                p += len;
            }
        }
    }
    if (fr <= d) return SamOverlap{-1, 0};  // no actual overlap
    const int64_t br = fr - d;
    int64_t bs = 0;
    p = 0;
    for (uint32_t k = 0; k < n1; k++) {
        const int64_t len = c1[k].count;
        const uint32_t t = c1[k].letter;
        if (len <= 0 && !err) err = kSamAssertCount;
        if (p < br) {
            if (t != 'D') bs += len < br - p ? len : br - p;
            if (t != 'I') p += len;
        }
    }
    const int64_t pos = d - ((fr - fs) - (br - bs));
    if (pos < 0) return SamOverlap{-1, 0};  // no acceptable overlap
    const int64_t a = len2 - pos;
    return SamOverlap{pos, a < len1 ? a : len1};
}

// the same for two alignments; CIGAR1 is read whole first (:276), then CIGAR2 (:278-280): a CIGAR the script cannot read kills it here
HC_SAM_HD SamOverlap sam_overlap_of(const hc_sam_aln& a1, const hc_sam_aln& a2, const hc_sam_op* ops, uint32_t& err) {
    const uint32_t bad = HC_SAM_CIGAR_VALUE_ERROR | HC_SAM_CIGAR_INDEX_ERROR;
    const uint32_t m = (a1.marks & bad) ? a1.marks : a2.marks;
    if ((m & bad) && !err) err = (m & HC_SAM_CIGAR_VALUE_ERROR) ? kSamCigarValue : kSamCigarIndex;
    if (err) return SamOverlap{-1, 0};
    return sam_overlap_pos(a1.cpos, a2.cpos, a1.len, a2.len, ops + a1.op_first, a1.op_count, ops + a2.op_first, a2.op_count, err);
}

// int(round(ovlen / min(len(seq1), len(seq2)) * 100)) under `from __future__ import division`, Python 2's round() = C round()
HC_SAM_HD int64_t sam_perc(int64_t ovlen, int64_t len_a, int64_t len_b, uint32_t& err) {
    const int64_t m = len_a < len_b ? len_a : len_b;
    if (m == 0) {
        if (!err) err = kSamZeroDivision;
        return 0;
    }
    const double q = round((double)ovlen / (double)m * 100.0);
    const int64_t perc = (int64_t)q;
    if ((perc < 0 || perc > 100) && !err) err = kSamAssertPerc;
    return perc;
}

struct SamPair {  // a record or an active read: its alignments, the pair's reverse mark
    uint32_t first, second, reverse;
};

// The line of (record, read), or none.  same_id: read's first id == record's second id (read only between two pairs, :361).
// src[0], src[1]: the alignments id1 and id2 come from.  err != 0: the script died here (the line is not valid).
HC_SAM_HD bool sam_pair_line(const hc_sam_aln* alns, const hc_sam_op* ops, const SamPair& record, const SamPair& read, int64_t mol, bool same_id,
                             hc_line_rec& out, uint32_t src[2], uint32_t& err) {
    const hc_sam_aln R = alns[record.first], Q = alns[read.first];
    const SamOverlap o1 = sam_overlap_of(R, Q, ops, err);
    if (err || o1.len <= mol || o1.pos < 0) return false;
    const bool rp = record.second != HC_SAM_NONE, qp = read.second != HC_SAM_NONE;
    const int64_t perc1 = sam_perc(o1.len, Q.len, R.len, err);
    if (err) return false;
    SamOverlap o2{0, 0};
    int64_t perc2 = 0;
    uint8_t ord = '-', ori1, ori2, t1 = 's', t2 = 's';
    if (!rp && !qp) {
        ori1 = (Q.flag & 16u) ? '-' : '+';
        ori2 = (R.flag & 16u) ? '-' : '+';
    } else {
        if (rp && !qp) {
            const hc_sam_aln R2 = alns[record.second];
            o2 = sam_overlap_of(R2, Q, ops, err);
            if (err) return false;
            perc2 = sam_perc(o2.len, Q.len, R2.len, err);
            t2 = 'p';
            ori1 = (Q.flag & 16u) ? '-' : '+';
            ori2 = record.reverse ? '-' : '+';
        } else if (!rp && qp) {
            const hc_sam_aln Q2 = alns[read.second];
            if (Q2.cpos - R.cpos < 0) return false;  // count_problems, :427-429
            o2 = sam_overlap_of(Q2, R, ops, err);
            if (err) return false;
            perc2 = sam_perc(o2.len, R.len, Q2.len, err);
            t2 = 'p';  // "s", "p" although id1 is the paired read, :438
            ori1 = read.reverse ? '-' : '+';
            ori2 = (R.flag & 16u) ? '-' : '+';
        } else {
            const hc_sam_aln R2 = alns[record.second], Q2 = alns[read.second];
            if (R2.cpos - Q2.cpos < 0) {
                o2 = sam_overlap_of(Q2, R2, ops, err);
                ord = same_id ? '1' : '2';
            } else {
                o2 = sam_overlap_of(R2, Q2, ops, err);
                ord = '1';
            }
            if (err) return false;
            perc2 = sam_perc(o2.len, R2.len, Q2.len, err);
            t1 = t2 = 'p';
            ori1 = read.reverse ? '-' : '+';
            ori2 = record.reverse ? '-' : '+';
        }
        if (err) return false;
        if (!(o2.len > mol && o2.pos >= 0)) return false;
    }
    const int64_t lim = 0xFFFFFFFFll;
    if (o1.pos > lim || o1.len > lim || o2.pos > lim || o2.len > lim) {
        err = kSamRange;
        return false;
    }
    out.id1 = (Q.marks & HC_SAM_ID_PLAIN) ? Q.id : read.first;
    out.id2 = (R.marks & HC_SAM_ID_PLAIN) ? R.id : record.first;
    out.pos1 = (uint32_t)o1.pos;
    out.pos2 = (uint32_t)o2.pos;
    out.perc1 = (uint32_t)perc1;
    out.perc2 = (uint32_t)perc2;
    out.len1 = (uint32_t)o1.len;
    out.len2 = (uint32_t)o2.len;
    out.ord = ord;
    out.ori1 = ori1;
    out.ori2 = ori2;
    out.type1 = t1;
    out.type2 = t2;
    out.pad[0] = out.pad[1] = out.pad[2] = 0;
    src[0] = read.first;
    src[1] = record.first;
    return true;
}

}  // namespace hc
