// hc_sr_fastq.h — what the kernels of hc_sr_fastq_kernels.hip and hc_api_sr_fastq.cpp share: the raw arrays of a store as the writers read
// them, the item layout of the four files and the launches.  The text of singles.fastq, paired1.fastq, paired2.fastq and
// removed_tip_sequences.fastq (reference src/SRBuilder.cpp:1386-1556) lies in ONE block, file after file.  Its items, file-major:
//     [0, n)        read r's record in singles.fastq      (0 characters for a paired read)
//     [n, 2 n)      read r's record in paired1.fastq      (0 for a single-end read)
//     [2 n, 3 n)    read r's record in paired2.fastq      (0 for a single-end read)
//     [3 n, 3 n + t) tip k's one or two records in removed_tip_sequences.fastq
//     3 n + t       the end
// so that one exclusive sum over the items' characters gives every record's place and, at entries 0, n, 2 n, 3 n and 3 n + t, the files'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hc {
namespace fastq {

struct Store {  // raw arrays on the device: off has n_seq + 1 entries, first n_reads + 1
    const uint8_t* bases;
    const uint8_t* quals;
    const uint64_t* off;
    const uint32_t* first;
    uint32_t n_reads;
};

struct Tips {  // tip k is read reads[k] of `store` (every entry below its n_reads: the host checked)
    Store store;
    const uint32_t* reads;
    uint64_t n;
};

// counters: n_records[4], then the five boundaries of the files in the block (n_bytes of file f = bound[f + 1] - bound[f])
enum { kCounterWords = 9 };

inline uint64_t n_items(uint32_t n_reads, uint64_t n_tips) { return 3ull * n_reads + n_tips; }

// sizes: n_items + 1 entries; counters: zeroed before the launch
hipError_t launch_sizes(Store cur, Tips tips, uint64_t* sizes, unsigned long long* counters, hipStream_t stream);
// pos: the exclusive sum of sizes; fills counters[4, 9)
hipError_t launch_bounds(uint32_t n_reads, uint64_t n_tips, const uint64_t* pos, unsigned long long* counters, hipStream_t stream);
hipError_t launch_write(Store cur, Tips tips, const uint64_t* pos, char* text, hipStream_t stream);

}  // namespace fastq
}  // namespace hc
