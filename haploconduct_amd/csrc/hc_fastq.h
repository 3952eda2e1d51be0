// hc_fastq.h — launch interface of hc_fastq_kernels.hip (the FASTQ files' text read on the device: hc_api_fastq.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hc {

// One file's text on the device.  line_start[k] = offset of line k's first byte for k <= 4 * (records read of it); line k ends in front of
// the newline at line_start[k + 1] - 1 when k + 1 <= n_newlines, else at n_bytes (a last line without a newline).  Offsets are 32 bits
// wide: a file has fewer than 2^32 - 4096 bytes (hcedge.h).
struct FastqFile {
    const char* text;
    const uint32_t* line_start;
    uint64_t n_bytes;
    uint32_t n_newlines;
};

// what a failed check leaves in first_bad: record << 3 | check (1, 2, 4, 5 of hcedge.h; check 3 is the host's); no failure: all ones
constexpr unsigned long long kFastqNoBad = ~0ull;

struct FastqRecordsOut {
    uint64_t* ids;        // by read: the id of a plain token (0 otherwise)
    uint32_t* tok_off;    // by read: the token's span in file 1's text
    uint32_t* tok_len;
    uint8_t* not_plain;   // by read: 1 = the host resolves the token
    uint64_t* lens;       // by sequence: the sequence line's length
    unsigned long long* first_bad;  // one word of this launch
    unsigned long long* n_not_plain;
};

// One lane per record of a file (paired: of both files): checks 1, 2, 4, 5, the token, a plain id, the lengths.  Read r of the launch is
// read first_read + r and owns sequences first_seq + r (single) or first_seq + 2 r, + 1 (pair).
hipError_t fastq_launch_records(const FastqFile& f1, const FastqFile& f2, bool paired, uint32_t n, uint32_t first_read, uint64_t first_seq,
                                const FastqRecordsOut& out, hipStream_t stream);

// One wave per sequence: its sequence line to bases + off[q], its quality line to quals + off[q].  Sequences [0, n_single) are records of
// file[0]; sequence n_single + 2 r + m is mate m of record r of file[1 + m].
struct FastqGather {
    FastqFile file[3];
    uint32_t n_single;
    uint64_t n_seq;
    const uint64_t* off;
    uint8_t* bases;
    uint8_t* quals;
};
hipError_t fastq_launch_gather(const FastqGather& g, hipStream_t stream);

// bases[i] = toupper(bases[i]) in the C locale (a-z only) for i < n_bytes; bases is 16-byte aligned
hipError_t fastq_launch_upper(uint8_t* bases, uint64_t n_bytes, uint32_t n_cu, hipStream_t stream);

}  // namespace hc
