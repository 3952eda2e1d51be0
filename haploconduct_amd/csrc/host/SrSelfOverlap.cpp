// SrSelfOverlap.cpp — host mirror of hc_sr_merge_self_overlaps (include/hcsr.h): SRBuilder::merge_self_overlap (reference
// src/SRBuilder.cpp:872-955) for a batch of pairs on plain base / quality arrays.  Own implementation; every pair is walked offset by
// offset and column by column as the reference does (SrSelfOverlap.h), on threads, so that the device's scan has something independent
// to be compared with.
#include "SrSelfOverlap.h"

#include <cstring>

#include "InBlocks.h"

extern "C" int hc_host_sr_merge_self_overlaps(const hc_settings* ec_settings, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes,
                                              const hc_sr_pair* pairs, uint64_t n_pairs, const hc_sr_self_settings* settings,
                                              int32_t* overlap_pos, double* score, uint32_t* status, uint64_t* out_off, uint8_t* merged_seq,
                                              uint8_t* merged_qual, uint64_t cap, uint64_t* n_out, hc_sr_self_stats* stats) {
    using namespace hc;
    if (!ec_settings || !settings || !out_off || !n_out || (n_pairs && (!pairs || !overlap_pos || !score || !status)) ||
        (n_bytes && (!seq || !qual)))
        return set_last_error(HC_ERR_ARG, "hc_host_sr_merge_self_overlaps: null argument");
    if (!(settings->min_qual == settings->min_qual)) return set_last_error(HC_ERR_ARG, "hc_host_sr_merge_self_overlaps: min_qual is NaN");
    if (stats) memset(stats, 0, sizeof *stats);
    *n_out = 0;
    out_off[0] = 0;
    if (n_pairs == 0) return HC_OK;
    const srself::Tables T(ec_settings->mismatch, ec_settings->min_read_len);
    struct Piece {
        std::vector<uint8_t> seq, qual;
    };
    const uint64_t block = 64, n_blocks = (n_pairs + block - 1) / block;
    std::vector<Piece> pieces(n_blocks);
    std::vector<uint32_t> lens(n_pairs);
    in_blocks(n_pairs, block, settings->n_threads, [&](uint64_t i0, uint64_t i1) {
        std::vector<uint8_t> s, q;
        Piece& P = pieces[i0 / block];
        for (uint64_t i = i0; i < i1; i++) {
            overlap_pos[i] = -1;
            score[i] = 0;
            lens[i] = 0;
            status[i] = srself::check_pair(seq, qual, n_bytes, pairs[i]);
            if (status[i] != HC_SR_SELF_NONE) continue;
            const hc_sr_pair& p = pairs[i];
            const srself::Mates M{seq + p.off1, qual + p.off1, seq + p.off2, qual + p.off2, p.len1, p.len2};
            overlap_pos[i] = srself::scan_pair(T, M, srself::first_offset(p.len1, settings->min_overlap), *settings, &score[i], s, q);
            if (overlap_pos[i] < 0) continue;
            status[i] = HC_SR_SELF_MERGED;
            lens[i] = (uint32_t)s.size();
            P.seq.insert(P.seq.end(), s.begin(), s.end());
            P.qual.insert(P.qual.end(), q.begin(), q.end());
        }
    });
    uint64_t total = 0, n_merged = 0, n_offsets = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        out_off[i] = total;
        total += lens[i];
        n_merged += status[i] == HC_SR_SELF_MERGED;
        if (status[i] <= HC_SR_SELF_MERGED) n_offsets += srself::first_offset(pairs[i].len1, settings->min_overlap);
    }
    out_off[n_pairs] = total;
    *n_out = total;
    if (stats) {
        stats->n_merged = n_merged;
        stats->n_offsets = n_offsets;
    }
    if (int rc = sr::check_room("hc_host_sr_merge_self_overlaps", "merged_seq / merged_qual", "n_out", total, cap, merged_seq, merged_qual)) return rc;
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (pieces[b].seq.empty()) continue;
        memcpy(merged_seq + out_off[b * block], pieces[b].seq.data(), pieces[b].seq.size());
        memcpy(merged_qual + out_off[b * block], pieces[b].qual.data(), pieces[b].qual.size());
    }
    return HC_OK;
}
