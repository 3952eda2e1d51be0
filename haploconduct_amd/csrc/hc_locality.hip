// hc_locality.hip — the locality order of a scoring launch.
//
// A candidate's partner rows are a random read of the store (the store holds the reads in file order, i.e. in random genome order), and
// at 10^8 candidates each one pulls its partner's two windows across the fabric on its own (45.8 GB per launch, L2 hit rate 0.44:
// profiles/traffic_c3.json of round 6).  Candidates whose hot reads lie next to each other on the genome have partners that lie next to
// each other too; scored together on one XCD, they find those rows in its L2.
//
//  * hc_set_reads: every read gets a key from its own bases — the smallest hashed 16-mer of mate /1 (of the read, for a single), round 5's
//    minimiser (tools/experiments/r05_layout_locality.py) — and the reads are sorted by it: `order` (reads in locality order).
//  * Per launch (launch_locality_index): overlap files are grouped by the smaller read id h = min(read1, read2) (scripts/sfo2overlaps.py:53),
//    so each hot read owns one contiguous run of records.  The run boundaries come from binary searches, one per read; the runs are then
//    laid out in `order` and `perm` lists the records run after run.  No record moves, and results go to each record's own index.
//
// Whatever the input, perm is a permutation of the launch's records: the boundaries are checked to be non-decreasing, and when they are
// not — or a sampled neighbour pair shows h decreasing — the batch is not grouped, the flag is set, perm is the identity and the scoring
// kernel, which reads the flag, scores the batch as given (hc_kernels.hip: score_kernel_coop, WQ).  The check decides speed, never results.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcedge.h"
#include "hc_prims.h"

namespace hc {

namespace {

constexpr uint32_t kLocK = 16;                                      // k-mer length: 2 bits a base fill 32 bits
constexpr uint64_t kLocHashMul = 0x9E3779B97F4A7C15ull;              // (Fibonacci hashing)
constexpr int kLocKeyBits = 44;                                     // keys are (k-mer * kLocHashMul mod 2^64) >> 20
constexpr uint64_t kLocNoKey = (1ull << kLocKeyBits) - 1;            // a sequence shorter than k
constexpr uint32_t kLocSamples = 1u << 16;                          // neighbour pairs the grouping check samples

__device__ __forceinline__ uint32_t base_code(uint8_t b) {  // A C G T -> 0 1 2 3; N and anything else -> 0 (a key, not a result)
    return b == 'C' ? 1u : (b == 'G' ? 2u : (b == 'T' ? 3u : 0u));
}

// One thread per read: the minimiser of its first sequence (mate /1, or the single read) over the bases as given.
__global__ __launch_bounds__(256) void locality_key_kernel(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ raw_off,
                                                           const uint32_t* __restrict__ read_first_seq, uint32_t n_reads,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t q = read_first_seq[r];
    const uint64_t off = raw_off[q], len = raw_off[q + 1] - off;
    uint64_t best = kLocNoKey;
    uint32_t kmer = 0;
    for (uint64_t j = 0; j < len; j++) {
        kmer = (kmer << 2) | base_code(bases[off + j]);
        if (j + 1 >= kLocK) {
            const uint64_t h = ((uint64_t)kmer * kLocHashMul) >> (64 - kLocKeyBits);
            best = h < best ? h : best;
        }
    }
    keys[r] = best;
    idx[r] = r;
}

__device__ __forceinline__ uint32_t hot_read(const void* in, uint64_t i, uint32_t n_reads) {  // min(read1, read2) of a compact record, clamped
    const uint2 p = *((const uint2*)((const hc_cand_rec*)in + i));
    const uint32_t h = p.x < p.y ? p.x : p.y;
    return h < n_reads ? h : n_reads;  // (ids out of range — records the kernel rejects — form one last run)
}

// bounds[h] = the first record whose hot read is >= h, h = 1 .. R (binary search); bounds[0] = 0, bounds[R + 1] = the number of records.
// The same grid samples kLocSamples neighbour pairs: h decreasing anywhere among them sets the flag.
__global__ __launch_bounds__(256) void locality_bounds_kernel(const void* __restrict__ in, uint64_t n, const unsigned long long* __restrict__ n_dev,
                                                              uint32_t n_reads, uint32_t* __restrict__ bounds, uint32_t* __restrict__ flag) {
    const uint64_t ne = n_dev ? (*n_dev < n ? *n_dev : n) : n;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_reads + 1u) {
        uint64_t b;
        if (t == 0) b = 0;
        else if (t == n_reads + 1u) b = ne;
        else {
            uint64_t lo = 0, hi = ne;  // hot_read(lo - 1) < t <= hot_read(hi) where the records are sorted
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (hot_read(in, mid, n_reads) < t) lo = mid + 1;
                else hi = mid;
            }
            b = lo;
        }
        bounds[t] = (uint32_t)b;
    }
    if (t < kLocSamples && ne >= 2) {
        const uint64_t i = (ne - 1) * t / kLocSamples;  // < ne - 1
        if (hot_read(in, i, n_reads) > hot_read(in, i + 1, n_reads)) atomicOr(flag, 1u);
    }
}

// len[k] = records of the k-th run in locality order (run R: out-of-range ids, last); boundaries that decrease set the flag.
__global__ __launch_bounds__(256) void locality_lengths_kernel(const uint32_t* __restrict__ order, uint32_t n_reads, const uint32_t* __restrict__ bounds,
                                                               uint32_t* __restrict__ len, uint32_t* __restrict__ flag) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_reads) return;
    const uint32_t h = k < n_reads ? order[k] : n_reads;
    const uint32_t lo = bounds[h], hi = bounds[h + 1];
    if (hi < lo) atomicOr(flag, 1u);
    len[k] = hi >= lo ? hi - lo : 0u;
}

// One wave per run: perm[start[k] + j] = bounds[h] + j.  Flag set: perm = the identity (any kernel that walks it still scores every record once).
__global__ __launch_bounds__(256) void locality_fill_kernel(const uint32_t* __restrict__ order, uint32_t n_reads, const uint32_t* __restrict__ bounds,
                                                            const uint32_t* __restrict__ start, const uint32_t* __restrict__ flag, uint64_t n,
                                                            const unsigned long long* __restrict__ n_dev, uint32_t* __restrict__ perm) {
    const uint64_t ne = n_dev ? (*n_dev < n ? *n_dev : n) : n;
    if (*flag) {
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += stride) perm[i] = (uint32_t)i;
        return;
    }
    const uint32_t k = (uint32_t)(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63u;
    if (k > n_reads) return;
    const uint32_t h = k < n_reads ? order[k] : n_reads;
    const uint32_t lo = bounds[h], len = bounds[h + 1] - lo, s = start[k];  // (flag clear: the boundaries do not decrease, the runs tile [0, ne))
    for (uint32_t j = lane; j < len; j += 64u)
        if ((uint64_t)s + j < ne) perm[s + j] = lo + j;
}

}  // namespace

size_t locality_order_temp_bytes(uint32_t n_reads) { return prims::sort_temp_bytes(n_reads, sizeof(uint64_t), sizeof(uint32_t)); }

// keys_a, keys_b: n_reads uint64 each; idx: n_reads uint32 (scratch); order_out: n_reads uint32.
hipError_t launch_locality_order(const uint8_t* bases, const uint64_t* raw_off, const uint32_t* read_first_seq, uint32_t n_reads, uint64_t* keys_a,
                                 uint64_t* keys_b, uint32_t* idx, uint32_t* order_out, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(locality_key_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, stream, bases, raw_off, read_first_seq, n_reads, keys_a, idx);
    // stable: reads of equal key keep their file order
    return prims::sort_pairs(temp, temp_bytes, keys_a, keys_b, idx, order_out, n_reads, 0, kLocKeyBits, stream);
}

size_t locality_index_temp_bytes(uint32_t n_reads) { return prims::scan_temp_bytes((uint64_t)n_reads + 1, sizeof(uint32_t)); }

// bounds: n_reads + 2 uint32; start: n_reads + 1 uint32; flag: one uint32; perm: n uint32 (entries from the device's count on are left alone).
hipError_t launch_locality_index(const uint32_t* order, uint32_t n_reads, const void* in, uint64_t n, const unsigned long long* n_dev, uint32_t* bounds,
                                 uint32_t* start, uint32_t* flag, uint32_t* perm, void* temp, size_t temp_bytes, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t threads = n_reads + 2u > kLocSamples ? n_reads + 2u : kLocSamples;
    hipLaunchKernelGGL(locality_bounds_kernel, dim3((threads + 255) / 256), dim3(256), 0, stream, in, n, n_dev, n_reads, bounds, flag);
    hipLaunchKernelGGL(locality_lengths_kernel, dim3((n_reads + 1u + 255) / 256), dim3(256), 0, stream, (const uint32_t*)order, n_reads,
                       (const uint32_t*)bounds, start, flag);
    e = prims::exclusive_sum(temp, temp_bytes, start, start, (uint64_t)n_reads + 1, stream);
    if (e != hipSuccess) return e;
    const uint64_t fill_threads = ((uint64_t)n_reads + 1) * 64;
    hipLaunchKernelGGL(locality_fill_kernel, dim3((uint32_t)((fill_threads + 255) / 256)), dim3(256), 0, stream, order, n_reads, (const uint32_t*)bounds,
                       (const uint32_t*)start, (const uint32_t*)flag, n, n_dev, perm);
    return hipGetLastError();
}

}  // namespace hc
