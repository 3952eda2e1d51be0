// SrFastq.cpp — hc_host_sr_fastq_text and hc_host_sr_fastq_tips_text (include/hcsr.h): the host mirrors of hc_sr_fastq_write_text.  The
// first is the record the three writers share (reference src/SRBuilder.cpp:1434-1447, :1484-1487, :1528-1535) over the reads of a store in
// ascending id, the second writeTipsToFile's loop (:1386-1414) over the reads the caller names.  Count, then fetch.
#include <cstring>
#include <string>

#include "../../../include/hcsr.h"
#include "../hc_ctx.h"

namespace {

int fail(const char* me, int status, const std::string& what) { return hc::set_last_error(status, std::string(me) + ": " + what); }

uint32_t digits(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) v /= 10, n++;
    return n;
}

// "@" id suffix "\n" SEQ "\n+\n" QUAL "\n"
uint64_t record_chars(uint64_t id, uint32_t suffix_chars, uint64_t len) { return 1 + digits(id) + suffix_chars + 1 + len + 3 + len + 1; }

char* put_record(char* p, uint64_t id, const char* suffix, const uint8_t* seq, const uint8_t* qual, uint64_t len) {
    const std::string head = "@" + std::to_string(id) + suffix + "\n";
    memcpy(p, head.data(), head.size());
    p += head.size();
    if (len) memcpy(p, seq, len);
    p += len;
    memcpy(p, "\n+\n", 3);
    p += 3;
    if (len) memcpy(p, qual, len);
    p += len;
    *p++ = '\n';
    return p;
}

const char* check_store(const uint64_t* seq_off, const uint32_t* first, uint32_t n_reads) {
    if (!seq_off || !first) return "null seq_off or read_first_seq";
    if (first[0] != 0 || seq_off[0] != 0) return "read_first_seq[0] or seq_off[0] is not 0";
    for (uint32_t r = 0; r < n_reads; r++) {
        const uint32_t k = first[r + 1] - first[r];
        if (first[r + 1] < first[r] || (k != 1 && k != 2)) return "a read must own 1 or 2 sequences";
    }
    for (uint32_t q = 0; q < first[n_reads]; q++)
        if (seq_off[q + 1] < seq_off[q]) return "seq_off descends";
    return nullptr;
}

}  // namespace

extern "C" int hc_host_sr_fastq_text(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                                     uint32_t n_reads, uint32_t file, char* text, uint64_t cap, uint64_t* n_bytes) {
    const char* me = "hc_host_sr_fastq_text";
    if (!n_bytes) return fail(me, HC_ERR_ARG, "null argument");
    *n_bytes = 0;
    if (file > HC_SR_FASTQ_PAIRED2) return fail(me, HC_ERR_ARG, "file is not 0, 1 or 2 (the tips: hc_host_sr_fastq_tips_text)");
    if (const char* what = check_store(seq_off, read_first_seq, n_reads)) return fail(me, HC_ERR_ARG, what);
    if (seq_off[read_first_seq[n_reads]] && (!bases || !quals)) return fail(me, HC_ERR_ARG, "null bases or quals");
    // which sequence of read r goes into this file, or none
    auto seq_of = [&](uint32_t r, uint32_t& q) {
        const bool paired = read_first_seq[r + 1] - read_first_seq[r] == 2;
        q = read_first_seq[r] + (file == HC_SR_FASTQ_PAIRED2 ? 1u : 0u);
        return paired == (file != HC_SR_FASTQ_SINGLES);
    };
    uint64_t total = 0;
    uint32_t q;
    for (uint32_t r = 0; r < n_reads; r++)
        if (seq_of(r, q)) total += record_chars(r, 0, seq_off[q + 1] - seq_off[q]);
    *n_bytes = total;
    if (total > cap || (total && !text)) return fail(me, HC_ERR_ARG, "text is missing or too small (n_bytes is filled)");
    char* p = text;
    for (uint32_t r = 0; r < n_reads; r++)  // outfile << "@" << ID << "\n" << seq << "\n" << "+\n" << phred << "\n", :1484-1487
        if (seq_of(r, q)) p = put_record(p, r, "", bases + seq_off[q], quals + seq_off[q], seq_off[q + 1] - seq_off[q]);
    return HC_OK;
}

extern "C" int hc_host_sr_fastq_tips_text(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                                          uint32_t n_reads, const uint32_t* tip_reads, uint64_t n_tips, char* text, uint64_t cap, uint64_t* n_bytes) {
    const char* me = "hc_host_sr_fastq_tips_text";
    if (!n_bytes) return fail(me, HC_ERR_ARG, "null argument");
    *n_bytes = 0;
    if (n_tips && !tip_reads) return fail(me, HC_ERR_ARG, "null tip_reads");
    if (const char* what = check_store(seq_off, read_first_seq, n_reads)) return fail(me, HC_ERR_ARG, what);
    if (seq_off[read_first_seq[n_reads]] && (!bases || !quals)) return fail(me, HC_ERR_ARG, "null bases or quals");
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_tips; k++) {
        const uint32_t r = tip_reads[k];
        if (r >= n_reads) return fail(me, HC_ERR_ARG, "a tip read is not below n_reads");
        const uint32_t q = read_first_seq[r];
        if (read_first_seq[r + 1] - q == 2) total += record_chars(k, 2, seq_off[q + 1] - seq_off[q]) + record_chars(k, 2, seq_off[q + 2] - seq_off[q + 1]);
        else total += record_chars(k, 0, seq_off[q + 1] - seq_off[q]);
    }
    *n_bytes = total;
    if (total > cap || (total && !text)) return fail(me, HC_ERR_ARG, "text is missing or too small (n_bytes is filled)");
    char* p = text;
    for (uint64_t k = 0; k < n_tips; k++) {  // new_ID = k, :1392-1411
        const uint32_t q = read_first_seq[tip_reads[k]];
        if (read_first_seq[tip_reads[k] + 1] - q == 2) {
            p = put_record(p, k, "_1", bases + seq_off[q], quals + seq_off[q], seq_off[q + 1] - seq_off[q]);
            p = put_record(p, k, "_2", bases + seq_off[q + 1], quals + seq_off[q + 1], seq_off[q + 2] - seq_off[q + 1]);
        } else {
            p = put_record(p, k, "", bases + seq_off[q], quals + seq_off[q], seq_off[q + 1] - seq_off[q]);
        }
    }
    return HC_OK;
}
