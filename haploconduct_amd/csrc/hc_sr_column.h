// hc_sr_column.h — one consensus column on the device (consensus_pos, reference src/SRBuilder.cpp:289-409), for sr_column_kernel
// (hc_sr_kernels.hip) and sr_self_merge_kernel (hc_sr_self_kernels.hip): the host-built log10 terms in LDS, the four sums and the table
// key that the members add to in list order, the base by exact comparison, the entry of a column of one or two members in the
// host-built table (include/hcsr.h: hc_host_sr_table) and the two output bytes.  No transcendental function runs here (DESIGN.md
// "Super-read consensus").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/SrCodes.h"

namespace hc {

static_assert(sr::kQDim == 128, "a table key holds (code, q) as code * 128 + q");

struct SrTerms {  // host/SrConsensus.h: terms, by term index; a workgroup's copy in LDS
    double same[sr::kQDim], other[sr::kQDim];
    __device__ inline void load(const double* __restrict__ terms) {  // by all lanes of the workgroup; the caller synchronises
        for (uint32_t i = threadIdx.x; i < sr::kQDim; i += blockDim.x) {
            same[i] = terms[i];
            other[i] = terms[sr::kQDim + i];
        }
    }
};

struct SrColumn {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;  // by base code A, C, G, T
    uint32_t cnt = 0, key = 0;              // members (N members too, :362); (code, q) of the first two, for the table

    // a member with base code <= kCodeN, quality q = byte - 33 (0 for an N) and term index ti
    __device__ inline void add(uint32_t code, uint32_t q, uint32_t ti, const SrTerms& T) {
        if (cnt < 2) key |= (code * 128u + q) << (cnt * 16);
        cnt++;
        if (code < 4) {  // :309-338: the member's term goes to all four scores
            const double a = T.same[ti], b = T.other[ti];
            s0 += code == 0 ? a : b;
            s1 += code == 1 ? a : b;
            s2 += code == 2 ? a : b;
            s3 += code == 3 ? a : b;
        }
    }
    __device__ inline double max_sum() const { return fmax(fmax(s0, s3), fmax(s1, s2)); }
    __device__ inline uint8_t nuc(double smax) const { return smax == s0 ? 'A' : (smax == s3 ? 'T' : (smax == s1 ? 'C' : 'G')); }  // :390-393
    // Phred, kEntryN or kEntryNaN of a column of one or two members; kEntryN for any other
    // Phred, kEntryN or kEntryNaN of a column of one member, and of two
    __device__ inline uint32_t entry1(const uint8_t* __restrict__ table) const { return table[sr::kTable1 + (key & 0xffffu)]; }
    __device__ inline uint32_t entry2(const uint8_t* __restrict__ table) const {
        const uint32_t k1 = key & 0xffffu, k2 = key >> 16;
        return table[(((k1 >> 7) * 5u + (k2 >> 7)) * 128u + (k1 & 127u)) * 128u + (k2 & 127u)];
    }
};

// the output bytes of a column with table entry (or Phred) `entry` and base `nuc`
__device__ inline void sr_put(uint32_t entry, uint8_t nuc, uint8_t& seq, uint8_t& qual) {
    seq = entry <= 93 ? nuc : (uint8_t)'N';
    qual = entry <= 93 ? (uint8_t)(entry + 33) : (uint8_t)'$';
}

}  // namespace hc
