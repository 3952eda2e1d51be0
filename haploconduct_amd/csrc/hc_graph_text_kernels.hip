// hc_graph_text_kernels.hip — the device side of hc_graph_write_text (include/hcedge.h): the bytes of graph.txt
// (OverlapGraph::writeGraphToFile, reference src/OverlapGraph.cpp:322-385), digraph.txt (writeDiGraphToFile, :388-409) and the GFA
// files (write2GFA, :468-543) from the adjacency lists in list order.  A fixed number of launches whatever the graph:
//
// decide_records_kernel (one lane per record) evaluates the reference's statements for its record: the skips, the asserts, whether a
//   line is written and how long it is.  graph.txt alone looks something up: for a record i -> j with j < i, checkEdge(j, i) (:233-247)
//   returns the score of the FIRST j -> i record of adj_out[j] in list order.  That scan is split as hc_trans_kernels.hip: k_list_sum and
//   the edge merge's getEdgeInfo scan are: a lane walks a list of fewer than 64 records, the wave walks a longer one 64 records at a
//   time and stops at the first chunk with a hit (ballot, lowest set lane), so a hub costs its list once.  The result — a keep byte and a
//   byte count per record — is all the write pass needs.  The counts (`count`, L_count, C_count) are workgroup tallies: one atomic each
//   per workgroup; a failed assert goes into one atomicMin on a packed key (hc_graph_text.h), which leaves the first in file order.
// decide_segments_kernel (GFA; a wave takes 64 segment vertices): the asserts of :494-508 in their order and the length of the S line;
//   the bytes of a reverse-complemented read are tested against build_rev_comp's alphabet with the same lane / wave split.
// One exclusive sum over the 64-bit byte counts places every item (hc_prims.hip).
// write_records_kernel (one lane per record) writes its line; lane 0 of workgroup 0 writes the header behind the scan.
// write_segments_kernel (GFA; one wave per segment) copies the read's bytes coalesced — 16-byte stores on 16-byte boundaries of the
//   text, head and tail bytewise, a reversed read back to front through build_rev_comp's mapping (hc_wave_copy.h).
// No atomics in the write pass, no libm anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_decimal.h"
#include "hc_graph_text.h"
#include "hc_wave_copy.h"

namespace hc {
namespace gtext {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNone = 0xffffffffu;

// The first k in [a, b) with E[k].v2 == target, or kNone; every lane of the wave calls it (a == b: nothing to find).
__device__ uint32_t find_first(const hc_edge_rec* __restrict__ E, uint32_t a, uint32_t b, uint32_t target, uint32_t lane) {
    uint32_t hit = kNone;
    const bool is_long = b - a >= 64;
    if (!is_long)
        for (uint32_t k = a; k < b; k++)
            if ((uint32_t)E[k].v2 == target) {
                hit = k;
                break;
            }
    unsigned long long longs = __ballot(is_long);
    while (longs) {
        const int j = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const uint32_t aj = __shfl(a, j), bj = __shfl(b, j), tj = __shfl(target, j);
        uint32_t found = kNone;
        for (uint32_t base = aj; base < bj; base += 64) {  // (wave-uniform: aj, bj and the ballot are)
            const uint32_t k = base + lane;
            const unsigned long long m = __ballot(k < bj && (uint32_t)E[k].v2 == tj);
            if (m) {
                found = base + (uint32_t)(__ffsll((long long)m) - 1);
                break;
            }
        }
        if ((int)lane == j) hit = found;
    }
    return hit;
}

__device__ __forceinline__ bool is_segment(const Reads& r, uint32_t v) { return v < r.n_singles || (v >= r.n_reads && v - r.n_reads < r.n_singles); }

// build_rev_comp (src/Types.h:109-129) appends for these five and exits on anything else
__device__ __forceinline__ bool rev_comp_known(uint8_t b) { return b == 'A' || b == 'T' || b == 'C' || b == 'G' || b == 'N'; }

// tally[t] += the lanes of the wave with pred (one LDS atomic per wave)
__device__ __forceinline__ void wave_tally(unsigned int* tally, bool pred, uint32_t lane) {
    const unsigned long long m = __ballot(pred);
    if (lane == 0 && m) atomicAdd(tally, (unsigned int)__popcll(m));
}

template <uint32_t KIND>
__global__ __launch_bounds__(kBlock) void decide_records_kernel(Graph g, Reads r, double edge_threshold, double merge_contigs,
                                                                uint64_t* __restrict__ sizes, uint8_t* __restrict__ keep,
                                                                unsigned long long* __restrict__ counters) {
    __shared__ unsigned int tally[3];  // pairs, links, contained
    __shared__ unsigned long long first_bad;
    if (threadIdx.x < 3) tally[threadIdx.x] = 0;
    if (threadIdx.x == 3) first_bad = kNoKey;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = k64 < g.n_edges;
    const uint32_t k = (uint32_t)k64;
    uint32_t i = 0, j = 0, pos = 0;
    if (valid) {
        i = (uint32_t)g.E[k].v1;  // (the owner of the list: hc_graph_load and hc_graph_resolve see to it)
        j = (uint32_t)g.E[k].v2;
        pos = k - (uint32_t)g.out_off[i];
    }
    uint32_t bytes = 0;
    bool kept = false, contained = false;
    uint64_t bad = kNoKey;
    if (KIND == HC_GRAPH_TEXT_CLIQUES) {
        bool look = false;
        if (valid) {
            if (g.incl[i]) bad = bad_key(i, 0, 1);  // :346, a status of the vertex
            else if (g.incl[j]) kept = false;       // :352
            else if (j == i) bad = bad_key(i, pos + 1, 0);  // :355
            else if (j < i) look = true;                    // :357
            else kept = true;
        }
        const uint32_t a = look ? (uint32_t)g.out_off[j] : 0u, b = look ? (uint32_t)g.out_off[j + 1] : 0u;
        const uint32_t f = find_first(g.E, a, b, i, lane);  // (every lane of the wave)
        if (look) {
            if (f == kNone) {
                kept = true;  // checkEdge returns -1
            } else {
                const double score = g.E[f].score, mismatch_rate = g.E[f].mismatch_rate;
                if (!(score >= edge_threshold || mismatch_rate <= merge_contigs)) bad = bad_key(i, pos + 1, 2);  // :242
                else kept = !(score > 0);
            }
        }
        if (kept) bytes = 2u * (digits_u32(i) + digits_u32(j) + 2u);  // "i,j\nj,i\n"
        wave_tally(&tally[0], kept, lane);
    } else if (KIND == HC_GRAPH_TEXT_DIGRAPH) {
        if (valid) {
            if (j == i) bad = bad_key(i, pos + 1, 0);  // :402
            else kept = true;
        }
        if (kept) bytes = digits_u32(i) + digits_u32(j) + 2u;  // "i\tj\n"
    } else {
        if (valid && is_segment(r, i)) {
            if (j == i) {
                bad = bad_key(i, pos + 1, 0);  // :513, before the filter
            } else if (is_segment(r, j)) {
                kept = true;
                contained = !(g.E[k].perc < 100);  // :519
                bytes = 10u + digits_u32(i) + digits_u32(j) + chars_i32(g.E[k].len0);  // "L\ti\t+\tj\t+\t" len0 "M\n"
            }
        }
        wave_tally(&tally[1], kept && !contained, lane);
        wave_tally(&tally[2], kept && contained, lane);
    }
    if (valid) {
        keep[k] = kept ? 1 : 0;
        sizes[KIND == HC_GRAPH_TEXT_GFA ? (uint64_t)k + i + 1u : (uint64_t)k] = bytes;
    }
    if (k64 == 0) sizes[n_items(KIND, g.V, g.n_edges)] = 0;
    if (bad != kNoKey) atomicMin(&first_bad, (unsigned long long)bad);
    __syncthreads();
    if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(&counters[threadIdx.x == 0 ? kPairs : threadIdx.x == 1 ? kLinks : kContained], (unsigned long long)tally[threadIdx.x]);
    if (threadIdx.x == 3 && first_bad != kNoKey) atomicMin(&counters[kKey], first_bad);
}

// segment s of 2 * n_singles: the vertex (s < n_singles: s itself, forwards; else n_reads + s - n_singles, reversed) and its read
__device__ __forceinline__ uint32_t segment_vertex(const Reads& r, uint32_t s) { return s < r.n_singles ? s : r.n_reads + (s - r.n_singles); }

__global__ __launch_bounds__(kBlock) void decide_segments_kernel(Graph g, Reads r, uint64_t* __restrict__ sizes,
                                                                 unsigned long long* __restrict__ counters) {
    __shared__ unsigned int tally;
    __shared__ unsigned long long first_bad;
    if (threadIdx.x == 0) tally = 0;
    if (threadIdx.x == 1) first_bad = kNoKey;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_seg = 2ull * r.n_singles;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock >> 6);
    for (uint64_t chunk = (uint64_t)blockIdx.x * (kBlock >> 6) + (threadIdx.x >> 6); chunk * 64 < n_seg; chunk += n_waves) {
        const uint64_t s = chunk * 64 + lane;
        const uint32_t v = s < n_seg ? segment_vertex(r, (uint32_t)s) : g.V;
        const bool valid = v < g.V;  // (V may end inside the reversed reads, or before them)
        const bool rev = s >= r.n_singles;
        uint64_t off = 0;
        uint32_t len = 0;
        uint64_t bad = kNoKey;
        bool scan = false;
        if (valid) {
            const uint32_t rd = rev ? v - r.n_reads : v, q = r.first[rd];
            if (r.first[rd + 1] - q != 1u) {
                bad = bad_key(v, 0, 1);  // :494, :500
            } else {
                off = r.off[q];
                len = (uint32_t)(r.off[q + 1] - off);
                if (len == 0) bad = bad_key(v, 0, 2);  // :508 (build_rev_comp of nothing is nothing)
                scan = rev && len != 0;
            }
        }
        // build_rev_comp's exit, ahead of :508: lanes walk the short reads, the wave walks each longer one 64 bytes at a time
        bool unknown = false;
        const bool is_long = scan && len >= 64;
        if (scan && !is_long)
            for (uint32_t t = 0; t < len; t++) unknown |= !rev_comp_known(r.bases[off + t]);
        unsigned long long longs = __ballot(is_long);
        while (longs) {
            const int jl = __ffsll((long long)longs) - 1;
            longs &= longs - 1;
            const uint64_t oj = __shfl(off, jl);
            const uint32_t lj = __shfl(len, jl);
            bool mine = false;
            for (uint32_t t = lane; t < lj; t += 64) mine |= !rev_comp_known(r.bases[oj + t]);
            const bool any = __ballot(mine) != 0ull;
            if ((int)lane == jl) unknown = any;
        }
        if (unknown) bad = bad_key(v, 0, 3);
        const bool ok = valid && bad == kNoKey;
        if (valid) sizes[g.out_off[v] + v] = ok ? 4u + digits_u32(v) + len : 0u;  // "S\t" v "\t" seq "\n"
        wave_tally(&tally, ok, lane);
        if (bad != kNoKey) atomicMin(&first_bad, (unsigned long long)bad);
    }
    __syncthreads();
    if (threadIdx.x == 0 && tally) atomicAdd(&counters[kSegments], (unsigned long long)tally);
    if (threadIdx.x == 1 && first_bad != kNoKey) atomicMin(&counters[kKey], first_bad);
}

template <uint32_t KIND>
__global__ __launch_bounds__(kBlock) void write_records_kernel(Graph g, const uint64_t* __restrict__ place, const uint8_t* __restrict__ keep,
                                                               const unsigned long long* __restrict__ counters, char* __restrict__ text) {
    const uint64_t k64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t header = 0;
    if (KIND == HC_GRAPH_TEXT_CLIQUES) {
        const uint64_t lines = 2ull * counters[kPairs];  // :373-374
        header = digits_u32(g.V) + digits_u64(lines) + 2u;
        if (k64 == 0) {
            char* p = put_u32(text, g.V);
            *p++ = '\n';
            p = put_u64(p, lines);
            *p = '\n';
        }
    } else if (KIND == HC_GRAPH_TEXT_GFA) {
        header = kGfaHeaderBytes;
        if (k64 == 0) {
            const char h[kGfaHeaderBytes + 1] = "H\tVN:Z:1.0\n";  // :478
            for (uint32_t t = 0; t < kGfaHeaderBytes; t++) text[t] = h[t];
        }
    }
    if (k64 >= g.n_edges) return;
    const uint32_t k = (uint32_t)k64;
    if (!keep[k]) return;
    const uint32_t i = (uint32_t)g.E[k].v1, j = (uint32_t)g.E[k].v2;
    char* p = text + header + place[KIND == HC_GRAPH_TEXT_GFA ? (uint64_t)k + i + 1u : (uint64_t)k];
    if (KIND == HC_GRAPH_TEXT_CLIQUES) {  // :362-365
        p = put_u32(p, i);
        *p++ = ',';
        p = put_u32(p, j);
        *p++ = '\n';
        p = put_u32(p, j);
        *p++ = ',';
        p = put_u32(p, i);
        *p = '\n';
    } else if (KIND == HC_GRAPH_TEXT_DIGRAPH) {  // :403
        p = put_u32(p, i);
        *p++ = '\t';
        p = put_u32(p, j);
        *p = '\n';
    } else {  // :520-521 and :525-526 write the same bytes
        *p++ = 'L';
        *p++ = '\t';
        p = put_u32(p, i);
        *p++ = '\t';
        *p++ = '+';
        *p++ = '\t';
        p = put_u32(p, j);
        *p++ = '\t';
        *p++ = '+';
        *p++ = '\t';
        p = put_i32(p, g.E[k].len0);
        *p++ = 'M';
        *p = '\n';
    }
}

// one wave per segment; only run when no assert failed, so every segment has one non-empty sequence
__global__ __launch_bounds__(kBlock) void write_segments_kernel(Graph g, Reads r, const uint64_t* __restrict__ place, char* __restrict__ text) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_seg = 2ull * r.n_singles;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock >> 6);
    for (uint64_t s = (uint64_t)blockIdx.x * (kBlock >> 6) + (threadIdx.x >> 6); s < n_seg; s += n_waves) {
        const uint32_t v = segment_vertex(r, (uint32_t)s);
        if (v >= g.V) continue;  // (wave-uniform)
        const bool rev = s >= r.n_singles;
        const uint32_t q = r.first[rev ? v - r.n_reads : v];
        const uint64_t off = r.off[q];
        const uint32_t len = (uint32_t)(r.off[q + 1] - off), dv = digits_u32(v);
        char* line = text + kGfaHeaderBytes + place[g.out_off[v] + v];
        if (lane == 0) {  // :509
            line[0] = 'S';
            line[1] = '\t';
            put_u32(line + 2, v);
            line[2 + dv] = '\t';
            line[3 + dv + len] = '\n';
        }
        uint8_t* d = (uint8_t*)line + 3 + dv;
        if (rev) wave_copy<true, true>(d, r.bases + off, len, lane);
        else wave_copy<false, false>(d, r.bases + off, len, lane);
    }
}

inline uint32_t record_grid(uint64_t n_edges) { return (uint32_t)((n_edges + kBlock - 1) / kBlock + (n_edges == 0)); }  // (n_edges < 2^31; one workgroup at least)
inline uint32_t wave_grid(uint64_t n_waves) {  // workgroups of four waves, at most 2^16 of them (the kernels stride)
    const uint64_t w = (n_waves + 3) / 4;
    return (uint32_t)(w < 1 ? 1 : (w > 65536 ? 65536 : w));
}

}  // namespace

hipError_t decide(uint32_t kind, const Graph& g, const Reads& r, double edge_threshold, double merge_contigs, uint64_t* sizes, uint8_t* keep,
                  unsigned long long* counters, hipStream_t stream) {
    const dim3 grid(record_grid(g.n_edges)), block(kBlock);
    if (kind == HC_GRAPH_TEXT_CLIQUES) {
        hipLaunchKernelGGL(decide_records_kernel<HC_GRAPH_TEXT_CLIQUES>, grid, block, 0, stream, g, r, edge_threshold, merge_contigs, sizes, keep, counters);
    } else if (kind == HC_GRAPH_TEXT_DIGRAPH) {
        hipLaunchKernelGGL(decide_records_kernel<HC_GRAPH_TEXT_DIGRAPH>, grid, block, 0, stream, g, r, edge_threshold, merge_contigs, sizes, keep, counters);
    } else {
        // the items of the vertices that are no segments stay 0
        const hipError_t e = hipMemsetAsync(sizes, 0, (n_items(kind, g.V, g.n_edges) + 1) * sizeof(uint64_t), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(decide_segments_kernel, dim3(wave_grid((2ull * r.n_singles + 63) / 64)), block, 0, stream, g, r, sizes, counters);
        hipLaunchKernelGGL(decide_records_kernel<HC_GRAPH_TEXT_GFA>, grid, block, 0, stream, g, r, edge_threshold, merge_contigs, sizes, keep, counters);
    }
    return hipGetLastError();
}

hipError_t write(uint32_t kind, const Graph& g, const Reads& r, const uint64_t* place, const uint8_t* keep, const unsigned long long* counters,
                 char* text, hipStream_t stream) {
    const dim3 grid(record_grid(g.n_edges)), block(kBlock);
    if (kind == HC_GRAPH_TEXT_CLIQUES) {
        hipLaunchKernelGGL(write_records_kernel<HC_GRAPH_TEXT_CLIQUES>, grid, block, 0, stream, g, place, keep, counters, text);
    } else if (kind == HC_GRAPH_TEXT_DIGRAPH) {
        hipLaunchKernelGGL(write_records_kernel<HC_GRAPH_TEXT_DIGRAPH>, grid, block, 0, stream, g, place, keep, counters, text);
    } else {
        hipLaunchKernelGGL(write_records_kernel<HC_GRAPH_TEXT_GFA>, grid, block, 0, stream, g, place, keep, counters, text);
        hipLaunchKernelGGL(write_segments_kernel, dim3(wave_grid(2ull * r.n_singles)), block, 0, stream, g, r, place, text);
    }
    return hipGetLastError();
}

}  // namespace gtext
}  // namespace hc
