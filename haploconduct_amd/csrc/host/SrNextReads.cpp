// SrNextReads.cpp — hc_host_sr_next_reads (include/hcsr.h): the host mirror of hc_sr_set_next_reads.  Which super-reads survive
// process_cliques (reference src/SRBuilder.cpp:983,986-996,999-1001), Read::get_len / test_N_rate (src/Read.h:203-234), the trivial
// super-reads with their reversal (src/SRBuilder.cpp:1282-1372) and the numbering across the three groups, entry by entry as the
// reference walks them, on plain arrays.  The entry's resolution and the tests are those the device runs (hc_sr_next.h).
#include <cstring>
#include <string>

#include "../../../include/hcsr.h"
#include "../hc_ctx.h"
#include "../hc_sr_next.h"

extern "C" int hc_host_sr_next_reads(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                                     uint32_t n_reads, const uint8_t* cons_seq, const uint8_t* cons_qual, uint64_t n_cons,
                                     const hc_sr_next_entry* entries, uint64_t n, const uint8_t* extra_seq, const uint8_t* extra_qual,
                                     uint64_t n_extra, const hc_sr_next_settings* settings, int32_t* new_id, uint32_t* status,
                                     hc_sr_next_counts* counts, uint8_t* out_bases, uint8_t* out_quals, uint64_t cap, uint64_t* n_bytes,
                                     uint64_t* out_seq_off, uint32_t* out_read_first_seq) {
    const char* me = "hc_host_sr_next_reads: ";
    if (!settings || !n_bytes || !out_seq_off || !out_read_first_seq || (n && (!entries || !new_id || !status)) ||
        (n_reads && (!seq_off || !read_first_seq)) || (n_cons && (!cons_seq || !cons_qual)) || (n_extra && (!extra_seq || !extra_qual)))
        return hc::set_last_error(HC_ERR_ARG, std::string(me) + "null argument");
    if (n >= (1ull << 31)) return hc::set_last_error(HC_ERR_ARG, std::string(me) + "2^31 entries or more");
    const hc::SrNextSources S{n_cons, n_extra, seq_off, read_first_seq, n_reads};
    const uint8_t* src_seq[3] = {cons_seq, extra_seq, bases};
    const uint8_t* src_qual[3] = {cons_qual, extra_qual, quals};
    hc_sr_next_counts cn;
    memset(&cn, 0, sizeof cn);
    // first the tests and the numbering, then — when there is room — the bytes
    for (int pass = 0; pass < 2; pass++) {
        uint64_t at = 0;
        uint32_t n_seq = 0, n_kept = 0;
        for (uint64_t i = 0; i < n; i++) {
            hc::SrNextResolved R;
            if (pass == 0) {
                uint32_t st = HC_SR_NEXT_BAD_ENTRY;
                if (hc::sr_next_resolve(entries[i], S, R)) {
                    uint64_t n_count = 0;
                    for (uint32_t k = 0; k < R.n_mates; k++)
                        for (uint32_t j = 0; j < R.m[k].len; j++) n_count += src_seq[R.m[k].src][R.m[k].off + j] == 'N';
                    st = hc::sr_next_status(entries[i].kind, R, n_count, settings->keep_singletons);
                }
                status[i] = st;
                new_id[i] = st == HC_SR_NEXT_KEPT ? (int32_t)n_kept : -1;
                cn.n_kept += st == HC_SR_NEXT_KEPT;
                cn.n_dropped_empty += st == HC_SR_NEXT_DROPPED_EMPTY;
                cn.n_dropped_n_rate += st == HC_SR_NEXT_DROPPED_N_RATE;
                cn.n_dropped_short += st == HC_SR_NEXT_DROPPED_SHORT;
                cn.n_bad += st == HC_SR_NEXT_BAD_ENTRY;
            }
            if (status[i] != HC_SR_NEXT_KEPT) continue;
            if (pass == 1) hc::sr_next_resolve(entries[i], S, R);
            out_read_first_seq[n_kept++] = n_seq;
            for (uint32_t k = 0; k < R.n_mates; k++) {
                const hc::SrNextMate& m = R.m[k];
                out_seq_off[n_seq++] = at;
                if (pass == 1) {
                    const uint8_t *sb = src_seq[m.src] + m.off, *sq = src_qual[m.src] + m.off;
                    if (R.rev) {
                        for (uint32_t j = 0; j < m.len; j++) {
                            out_bases[at + j] = hc::sr_next_complement(sb[m.len - 1 - j]);
                            out_quals[at + j] = sq[m.len - 1 - j];
                        }
                    } else if (m.len) {
                        memcpy(out_bases + at, sb, m.len);
                        memcpy(out_quals + at, sq, m.len);
                    }
                }
                at += m.len;
            }
        }
        out_read_first_seq[n_kept] = n_seq;
        out_seq_off[n_seq] = at;
        if (pass == 0) {
            cn.n_seq = n_seq;
            cn.n_bytes = at;
            *n_bytes = at;
            if (counts) *counts = cn;
            if (n_kept == 0) return HC_SR_NEXT_EMPTY;
            if (cap < at || !out_bases || !out_quals)
                return hc::set_last_error(HC_ERR_ARG, std::string(me) + "out_bases / out_quals too small (n_bytes holds the need)");
        }
    }
    return HC_OK;
}
