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
//    so each hot read owns one contiguous run of records.  The run boundaries come from binary searches, one per read (bounds); the runs
//    are then laid out in `order` — their lengths summed per tile of 512 runs (sums), a tile's first slot being the sum of the tiles in
//    front of it and the starts inside a tile a scan in its workgroup (fill) — and `perm` lists the records run after run: three launches,
//    none of which waits for another workgroup.  No record moves, and results go to each record's own index.
//
// Whatever the input, perm is a permutation of the launch's records: the boundaries are checked to be non-decreasing — a sequence that is
// non-decreasing from 0 to the number of records tiles the records, whatever its entries mean — and when they are not, or a sampled
// neighbour pair shows h decreasing, the batch is not grouped, the flag is set, perm is the identity and the scoring kernel, which reads
// the flag, scores the batch as given (hc_kernels.hip: score_kernel_coop, WQ).  The check decides speed, never results.
//
// Measured and not kept (profiles/r09_item_feed.md): boundaries from one thread per block of 64 records (4 x the searches' time) and a
// fill from the slots' side with 16-byte stores (1.6 x the time of one wave per run).
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
constexpr uint32_t kLocTileRuns = 512;                              // runs per workgroup of the sums and the fill kernel

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
// The flag is zeroed here — this kernel does not set it — and set by the sums kernel, which runs behind it (no hipMemsetAsync).
__global__ __launch_bounds__(256) void locality_bounds_kernel(const void* __restrict__ in, uint64_t n, const unsigned long long* __restrict__ n_dev,
                                                              uint32_t n_reads, uint32_t* __restrict__ bounds, uint32_t* __restrict__ flag) {
    const uint64_t ne = n_dev ? (*n_dev < n ? *n_dev : n) : n;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_reads + 1u) {
        uint64_t b;
        if (t == 0) {
            b = 0;
            *flag = 0;
        } else if (t == n_reads + 1u) {
            b = ne;
        } else {
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
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// The runs in locality order (run R: out-of-range ids, last), kLocTileRuns of them per workgroup: tile_sum[t] = the records of tile t's
// runs.  Boundaries that decrease set the flag, and so does h decreasing anywhere among kLocSamples sampled neighbour pairs, which the
// same grid looks at.
__global__ __launch_bounds__(256) void locality_sums_kernel(const uint32_t* __restrict__ order, uint32_t n_reads, const uint32_t* __restrict__ bounds,
                                                            const void* __restrict__ in, uint64_t n, const unsigned long long* __restrict__ n_dev,
                                                            uint32_t* __restrict__ tile_sum, uint32_t* __restrict__ flag) {
    __shared__ uint32_t part[4];
    const uint64_t ne = n_dev ? (*n_dev < n ? *n_dev : n) : n;
    uint32_t sum = 0;
    bool bad = false;
    if (ne >= 2)
        for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < kLocSamples; t += gridDim.x * 256u) {
            const uint64_t i = (ne - 1) * t / kLocSamples;  // < ne - 1
            bad |= hot_read(in, i, n_reads) > hot_read(in, i + 1, n_reads);
        }
    for (uint32_t j = threadIdx.x; j < kLocTileRuns; j += 256u) {
        const uint64_t k = (uint64_t)blockIdx.x * kLocTileRuns + j;
        if (k > n_reads) break;
        const uint32_t h = k < n_reads ? order[k] : n_reads;
        const uint32_t lo = bounds[h], hi = bounds[h + 1];
        bad |= hi < lo;
        sum += hi >= lo ? hi - lo : 0u;
    }
    if (bad) atomicOr(flag, 1u);
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// One workgroup per tile of runs: the tile's first slot is the sum of the tiles in front of it, the runs' starts come from a scan inside
// the workgroup, and its waves take the tile's runs in turn: perm[start[k] + j] = bounds[h] + j.  Flag set: perm = the identity (any
// kernel that walks it still scores every record once).
__global__ __launch_bounds__(256) void locality_fill_kernel(const uint32_t* __restrict__ order, uint32_t n_reads, const uint32_t* __restrict__ bounds,
                                                            const uint32_t* __restrict__ tile_sum, uint32_t n_tiles, const uint32_t* __restrict__ flag,
                                                            uint64_t n, const unsigned long long* __restrict__ n_dev, uint32_t* __restrict__ perm) {
    const uint64_t ne = n_dev ? (*n_dev < n ? *n_dev : n) : n;
    if (*flag) {
        const uint64_t stride = 4ull * gridDim.x * blockDim.x;
        for (uint64_t i = 4ull * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); i < ne; i += stride) {
            if (i + 4 <= ne) *(uint4*)(perm + i) = uint4{(uint32_t)i, (uint32_t)i + 1u, (uint32_t)i + 2u, (uint32_t)i + 3u};
            else
                for (uint64_t p = i; p < ne; ++p) perm[p] = (uint32_t)p;
        }
        return;
    }
    if (blockIdx.x >= n_tiles) return;  // (the grid is wide enough for the identity whatever the number of reads)
    __shared__ uint32_t s_start[kLocTileRuns + 1], s_lo[kLocTileRuns], part[8];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t base = 0;
    for (uint32_t j = t; j < blockIdx.x; j += 256u) base += tile_sum[j];
    base = wave_sum(base);
    // thread t owns the tile's runs 2 t and 2 t + 1 (flag clear: the boundaries do not decrease, the runs tile [0, ne))
    uint32_t lo[2] = {0, 0}, len[2] = {0, 0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint64_t k = (uint64_t)blockIdx.x * kLocTileRuns + 2u * t + q;
        if (k <= n_reads) {
            const uint32_t h = k < n_reads ? order[k] : n_reads;
            lo[q] = bounds[h];
            len[q] = bounds[h + 1] - lo[q];
        }
    }
    uint32_t incl = len[0] + len[1];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
        if ((int)lane >= o) incl += up;
    }
    if (lane == 63u) part[4 + wave] = incl;
    if (lane == 0u) part[wave] = base;
    __syncthreads();
    uint32_t excl = part[0] + part[1] + part[2] + part[3] + incl - (len[0] + len[1]);
    for (uint32_t w = 0; w < wave; ++w) excl += part[4 + w];
    s_start[2u * t] = excl;
    s_start[2u * t + 1u] = excl + len[0];
    s_lo[2u * t] = lo[0];
    s_lo[2u * t + 1u] = lo[1];
    if (t == 255u) s_start[kLocTileRuns] = excl + len[0] + len[1];
    __syncthreads();
    for (uint32_t r = wave; r < kLocTileRuns; r += 4u) {  // a wave per run
        const uint32_t s = s_start[r], len = s_start[r + 1u] - s, l0 = s_lo[r];
        for (uint32_t j = lane; j < len; j += 64u)
            if ((uint64_t)s + j < ne) perm[s + j] = l0 + j;
    }
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

static uint32_t locality_tiles(uint32_t n_reads) { return (uint32_t)(((uint64_t)n_reads + 1 + kLocTileRuns - 1) / kLocTileRuns); }

size_t locality_index_work_words(uint32_t n_reads) { return locality_tiles(n_reads); }  // the tiles' sums

// bounds: n_reads + 2 uint32; work: locality_index_work_words(n_reads) uint32; flag: one uint32; perm: n uint32, 16-byte aligned (entries
// from the device's count on are left alone).  Three launches, none of which waits for another workgroup.
hipError_t launch_locality_index(const uint32_t* order, uint32_t n_reads, const void* in, uint64_t n, const unsigned long long* n_dev, uint32_t* bounds,
                                 uint32_t* work, uint32_t* flag, uint32_t* perm, hipStream_t stream) {
    const uint32_t tiles = locality_tiles(n_reads);
    hipLaunchKernelGGL(locality_bounds_kernel, dim3((n_reads + 2u + 255) / 256), dim3(256), 0, stream, in, n, n_dev, n_reads, bounds, flag);
    hipLaunchKernelGGL(locality_sums_kernel, dim3(tiles), dim3(256), 0, stream, order, n_reads, (const uint32_t*)bounds, in, n, n_dev, work, flag);
    const uint64_t wide = (n + 4095) / 4096 < 1024 ? (n + 4095) / 4096 : 1024;  // workgroups for the identity of a batch that is not grouped
    hipLaunchKernelGGL(locality_fill_kernel, dim3(tiles > wide ? tiles : (uint32_t)wide), dim3(256), 0, stream, order, n_reads, (const uint32_t*)bounds,
                       (const uint32_t*)work, tiles, (const uint32_t*)flag, n, n_dev, perm);
    return hipGetLastError();
}

}  // namespace hc
