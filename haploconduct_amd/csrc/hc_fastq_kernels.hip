// hc_fastq_kernels.hip — the FASTQ files' text on the device (hc_fastq.h; the call is hc_api_fastq.cpp: hc_set_reads_from_fastq_text).
//   fastq_records_kernel   one lane per record: the reader's checks 1, 2, 4, 5 (hcedge.h), the header's token, a plain id, the lengths
//   fastq_gather_kernel    one wave per sequence: the sequence and the quality line to their places in the raw arrays (hc_wave_copy.h)
//   fastq_upper_kernel     the singles' bases through toupper, 16 bytes a lane
// The line starts come from hc_text_kernels.hip (newlines per 4 KiB tile, one sum, the starts).  Byte movers bound by HBM: no LDS table,
// nothing but plain loads and stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hc_fastq.h"
#include "hc_wave_copy.h"

namespace hc {

__device__ __forceinline__ void fastq_line(const FastqFile& f, uint64_t k, uint32_t& at, uint32_t& len) {
    at = f.line_start[k];
    const uint32_t end = k + 1 <= (uint64_t)f.n_newlines ? f.line_start[k + 1] - 1u : (uint32_t)f.n_bytes;
    len = end - at;
}

// isspace in the C locale
__device__ __forceinline__ bool fastq_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

// `stream >> id` on the header without its first character (host_model.cpp: first_token)
__device__ __forceinline__ void fastq_token(const char* s, uint32_t n, uint32_t& a, uint32_t& len) {
    a = n ? 1u : 0u;
    while (a < n && fastq_space((uint8_t)s[a])) a++;
    uint32_t b = a;
    while (b < n && !fastq_space((uint8_t)s[b])) b++;
    len = b - a;
}

__global__ __launch_bounds__(256) void fastq_records_kernel(FastqFile f1, FastqFile f2, uint32_t paired, uint32_t n, uint32_t first_read,
                                                            uint64_t first_seq, FastqRecordsOut out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    uint32_t check = 0, flag = 0;
    if (r < n) {
        uint32_t h1, hn1, s1, sn1, q1, qn1, h2 = 0, hn2 = 0, s2 = 0, sn2 = 0, q2 = 0, qn2 = 0;
        fastq_line(f1, 4ull * r, h1, hn1);
        fastq_line(f1, 4ull * r + 1, s1, sn1);
        fastq_line(f1, 4ull * r + 3, q1, qn1);
        if (paired) {
            fastq_line(f2, 4ull * r, h2, hn2);
            fastq_line(f2, 4ull * r + 1, s2, sn2);
            fastq_line(f2, 4ull * r + 3, q2, qn2);
        }
        uint32_t ta = 0, tn = 0;
        uint64_t id = 0;
        if (hn1 == 0 || f1.text[h1] != '@') {
            check = 1;
        } else {
            const char* t1 = f1.text + h1;
            fastq_token(t1, hn1, ta, tn);
            if (paired) {
                const char* t2 = f2.text + h2;
                uint32_t tb, tm;
                fastq_token(t2, hn2, tb, tm);
                bool same = tn == tm;
                for (uint32_t i = 0; same && i < tn; i++) same = t1[ta + i] == t2[tb + i];
                if (!same) check = 2;
            }
            if (!check) {
                // parse_id's fast path: 0 or [1-9][0-9]{0,17}
                bool plain = tn >= 1 && tn <= 18 && (t1[ta] != '0' || tn == 1);
                for (uint32_t i = 0; plain && i < tn; i++) {
                    const uint32_t d = (uint32_t)(uint8_t)t1[ta + i] - (uint32_t)'0';
                    plain = d <= 9u;
                    id = id * 10u + d;
                }
                if (!plain) id = 0, flag = 1;
                if (sn1 == 0 || (paired && sn2 == 0)) check = 4;
                else if (sn1 != qn1 || (paired && sn2 != qn2)) check = 5;
            }
        }
        const uint32_t read = first_read + r;
        out.ids[read] = id;
        out.tok_off[read] = h1 + ta;
        out.tok_len[read] = tn;
        out.not_plain[read] = (uint8_t)flag;
        if (paired) {
            out.lens[first_seq + 2ull * r] = sn1;
            out.lens[first_seq + 2ull * r + 1] = sn2;
        } else {
            out.lens[first_seq + r] = sn1;
        }
    }
    // the first bad record of the launch, the tokens left to the host: one atomic a wave where there is something to say
    const unsigned long long bad = __ballot(check != 0), np = __ballot(flag != 0);
    const uint32_t lane = threadIdx.x & 63u;
    if (bad && lane == (uint32_t)__builtin_ctzll(bad)) atomicMin(out.first_bad, (unsigned long long)r << 3 | check);  // lanes ascend with r
    if (np && lane == 0) atomicAdd(out.n_not_plain, (unsigned long long)__builtin_popcountll(np));
}

__global__ __launch_bounds__(256) void fastq_gather_kernel(FastqGather g) {
    const uint64_t q = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (q >= g.n_seq) return;
    uint32_t which = 0;
    uint64_t r = q;
    if (q >= g.n_single) {
        const uint64_t p = q - g.n_single;
        which = 1u + (uint32_t)(p & 1u);
        r = p >> 1;
    }
    const FastqFile& f = g.file[which];
    uint32_t s, sn, ql, qn;
    fastq_line(f, 4ull * r + 1, s, sn);
    fastq_line(f, 4ull * r + 3, ql, qn);  // (qn == sn: check 5 passed before this launch)
    const uint64_t o = g.off[q];
    wave_copy<false, false>(g.bases + o, (const uint8_t*)f.text + s, sn, lane);
    wave_copy<false, false>(g.quals + o, (const uint8_t*)f.text + ql, sn, lane);
}

// bytes a..z of w less 0x20, every other byte as it is
__device__ __forceinline__ uint32_t fastq_upper4(uint32_t w) {
    const uint32_t low = w & 0x7F7F7F7Fu;
    const uint32_t ge_a = low + 0x1F1F1F1Fu;  // bit 7 of a byte: its low seven bits >= 0x61
    const uint32_t gt_z = low + 0x05050505u;  // ... >= 0x7B
    const uint32_t m = ge_a & ~gt_z & ~w & 0x80808080u;
    return w - (m >> 2);
}

__global__ __launch_bounds__(256) void fastq_upper_kernel(uint8_t* __restrict__ bases, uint64_t n_bytes) {
    const uint64_t n_vec = n_bytes >> 4, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < n_vec; v += stride) {
        uint4 w = *(const uint4*)(bases + (v << 4));
        w = make_uint4(fastq_upper4(w.x), fastq_upper4(w.y), fastq_upper4(w.z), fastq_upper4(w.w));
        *(uint4*)(bases + (v << 4)) = w;
    }
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(n_bytes & 15u)) {
        const uint64_t i = (n_vec << 4) + threadIdx.x;
        const uint8_t b = bases[i];
        if (b >= 'a' && b <= 'z') bases[i] = (uint8_t)(b - 0x20u);
    }
}

hipError_t fastq_launch_records(const FastqFile& f1, const FastqFile& f2, bool paired, uint32_t n, uint32_t first_read, uint64_t first_seq,
                                const FastqRecordsOut& out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fastq_records_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, f1, f2, paired ? 1u : 0u, n, first_read, first_seq, out);
    return hipGetLastError();
}

hipError_t fastq_launch_gather(const FastqGather& g, hipStream_t stream) {
    if (g.n_seq == 0) return hipSuccess;
    hipLaunchKernelGGL(fastq_gather_kernel, dim3((uint32_t)((g.n_seq + 3) / 4)), dim3(256), 0, stream, g);
    return hipGetLastError();
}

hipError_t fastq_launch_upper(uint8_t* bases, uint64_t n_bytes, uint32_t n_cu, hipStream_t stream) {
    if (n_bytes == 0) return hipSuccess;
    const uint64_t want = ((n_bytes >> 4) + 255) / 256;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)n_cu * 16));
    hipLaunchKernelGGL(fastq_upper_kernel, dim3(grid), dim3(256), 0, stream, bases, n_bytes);
    return hipGetLastError();
}

}  // namespace hc
