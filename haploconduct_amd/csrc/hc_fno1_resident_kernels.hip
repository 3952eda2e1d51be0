// hc_fno1_resident_kernels.hip — the device side of hc_fno1_from_graph (include/hcsr.h): the edge list SRBuilder::findNextOverlaps walks
// (reference src/FindNextOverlaps.cpp:612-630, :635-813, :816-887), built from the graph the context holds.  The walk itself, the sorts
// and the text are hc_fno_kernels.hip's.  One lane per item, except where checkEdge meets a long out-list; no atomics on the outputs
// (the status word is an atomicOr of bits).
//
// f1r_convert_kernel        80-byte graph record k -> hc_fno_edge k, 16-byte loads and stores.
// f1r_group_pairs_kernel    group g -> l (l - 1) / 2.
// f1r_nonedge_lanes_kernel  stored non-edge i -> keep / long; f1r_nonedge_waves_kernel: the long ones, a wave each.
// f1r_induced_lanes_kernel  pair t -> its group (bisection), (i, j) (hc_fno1_induced.h), the induced edge, keep / long;
// f1r_induced_waves_kernel  the long ones; f1r_induced_build_kernel: survivor k -> its edge.
// f1r_cliques_kernel, f1r_subread_keys_kernel, f1r_subread_gather_kernel: the super-read tables.
// f1r_line_heads_kernel, f1r_line_records_kernel: the unique lines as hc_line_rec.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_fno1_induced.h"
#include "hc_fno1_resident.h"
#include "hc_fno_device.h"

namespace hc {
namespace fno1r {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * kBlock + threadIdx.x; }
dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// the largest j in [0, n) with a[j] <= x, for a[0] <= x < a[n] and ascending a
__device__ inline uint64_t owner(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

static_assert(sizeof(hc_edge_rec) == 80 && sizeof(hc_fno_edge) == 48, "the conversion moves five and three 16-byte words");
__global__ __launch_bounds__(kBlock) void f1r_convert_kernel(const hc_edge_rec* __restrict__ in, uint64_t n, hc_fno_edge* __restrict__ out) {
    const uint64_t k = gid();
    if (k >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(in + k);
    const uint4 q0 = src[0];  // score | mismatch_rate
    const uint4 q1 = src[1];  // pos1 pos2 | pos3 pos4
    const uint4 q2 = src[2];  // ori1 ori2 ord pad | read1 | read2 | (padding)
    const uint4 q3 = src[3];  // v1 | v2
    const uint4 q4 = src[4];  // perc len0 | len1 len2
    const uint32_t ori1 = q2.x & 0xFFu, ori2 = (q2.x >> 8) & 0xFFu, ord = (q2.x >> 16) & 0xFFu;
    uint4* dst = reinterpret_cast<uint4*>(out + k);
    dst[0] = q3;                                                // v1 | v2
    dst[1] = make_uint4(q0.x, q0.y, q1.x, q1.y);                // score | pos1 pos2
    dst[2] = make_uint4(q4.z, q4.w, q4.x, ord | ori1 << 8 | ori2 << 16);  // len1 len2 | perc, ord ori1 ori2 pad
}

__global__ __launch_bounds__(kBlock) void f1r_group_pairs_kernel(const uint64_t* __restrict__ off, uint64_t n_groups, uint64_t* __restrict__ cnt) {
    const uint64_t g = gid();
    if (g > n_groups) return;
    cnt[g] = g < n_groups ? fno1i::pairs_of(off[g + 1] - off[g]) : 0;
}

// ---- OverlapGraph::checkEdge(v, w, true), src/OverlapGraph.cpp:233-259 -----------------------------------------------------------------
// The score of the first edge v -> w in v's list, else of the first w -> v in w's list, else -1.  One function, two forms: a lane alone
// for short lists, a wave for long ones (64 records at a time, stopping at the first chunk with a hit); both answer with the same record.
__device__ inline bool lists_are_short(const Adj& a, uint64_t v, uint64_t w) {
    return a.out_off[v + 1] - a.out_off[v] < kLaneList && a.out_off[w + 1] - a.out_off[w] < kLaneList;
}
__device__ inline double check_edge_lane(const Adj& a, uint64_t v, uint64_t w) {
    for (uint64_t k = a.out_off[v], e = a.out_off[v + 1]; k < e; ++k)
        if (a.edges[k].v2 == w) return a.edges[k].score;
    for (uint64_t k = a.out_off[w], e = a.out_off[w + 1]; k < e; ++k)
        if (a.edges[k].v2 == v) return a.edges[k].score;
    return -1.0;
}
__device__ inline bool first_hit_wave(const Adj& a, uint64_t from, uint64_t to, unsigned lane, double* score) {  // the whole wave calls it
    for (uint64_t c = a.out_off[from], e = a.out_off[from + 1]; c < e; c += 64) {
        const uint64_t k = c + lane;
        const bool hit = k < e && a.edges[k].v2 == to;
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            *score = a.edges[c + (uint64_t)(__ffsll((long long)mask) - 1)].score;
            return true;
        }
    }
    return false;
}
__device__ inline double check_edge_wave(const Adj& a, uint64_t v, uint64_t w, unsigned lane) {
    double score = -1.0;
    if (first_hit_wave(a, v, w, lane, &score)) return score;
    if (first_hit_wave(a, w, v, lane, &score)) return score;
    return -1.0;
}
__device__ inline uint8_t nonedge_kept(double r) { return r > 0 ? 0 : 1; }      // :694: `checkEdge(...) > 0` drops the line
__device__ inline uint8_t induced_kept(double r) { return r == -1 ? 1 : 0; }   // :876: `checkEdge(...) == -1` keeps the edge

// 0: the record is looked up; else the status bit it sets
__device__ inline unsigned long long nonedge_status(const hc_fno_edge& e, uint64_t n_nodes) {
    if (e.score != 0) return kFnoStatusRange;  // not a stored non-edge: the host form says so
    if (!(e.len1 > 0 && e.len2 >= 0) || e.v1 >= n_nodes || e.v2 >= n_nodes) return kFnoStatusRequire;  // Edge::set_len, a vertex the graph lacks
    return 0;
}

__global__ __launch_bounds__(kBlock) void f1r_nonedge_lanes_kernel(const hc_fno_edge* __restrict__ non, uint64_t n, Adj a, uint8_t* __restrict__ keep,
                                                                   uint8_t* __restrict__ is_long, unsigned long long* __restrict__ status) {
    const uint64_t i = gid();
    if (i >= n) return;
    const hc_fno_edge e = non[i];
    uint8_t k = 0, l = 0;
    if (const unsigned long long bad = nonedge_status(e, a.n_nodes)) atomicOr(&status[4], bad);
    else if (lists_are_short(a, e.v1, e.v2)) k = nonedge_kept(check_edge_lane(a, e.v1, e.v2));
    else l = 1;
    keep[i] = k;
    is_long[i] = l;
}

__global__ __launch_bounds__(kBlock) void f1r_nonedge_waves_kernel(const hc_fno_edge* __restrict__ non, const uint32_t* __restrict__ long_idx,
                                                                   const unsigned long long* __restrict__ n_long, Adj a, uint8_t* __restrict__ keep) {
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / 64, n_waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t n = *n_long;
    for (uint64_t k = wave; k < n; k += n_waves) {
        const uint32_t i = long_idx[k];
        const hc_fno_edge e = non[i];  // (long only where nonedge_status passed)
        const double r = check_edge_wave(a, e.v1, e.v2, lane);
        if (lane == 0) keep[i] = nonedge_kept(r);
    }
}

// pair t -> the induced edge (hc_fno1_induced.h) or why there is none
__device__ inline int induced_of(const Groups& g, const Adj& a, uint64_t t, hc_fno_edge* ne) {
    const uint64_t grp = owner(g.pair_off, g.n_groups, t);
    const uint64_t first = g.off[grp], l = g.off[grp + 1] - first;
    uint32_t i, j;
    fno1i::pair_of(t - g.pair_off[grp], l, &i, &j);
    return fno1i::induced_edge(g.edges[first + i], g.edges[first + j], a.nodes, a.n_nodes, g.edge_threshold, ne);
}

__global__ __launch_bounds__(kBlock) void f1r_induced_lanes_kernel(Groups g, uint64_t n_pairs, Adj a, uint8_t* __restrict__ keep,
                                                                   uint8_t* __restrict__ is_long, unsigned long long* __restrict__ status) {
    const uint64_t t = gid();
    if (t >= n_pairs) return;
    hc_fno_edge ne;
    const int verdict = induced_of(g, a, t, &ne);
    uint8_t k = 0, l = 0;
    if (verdict >= fno1i::kStopRelation) atomicOr(&status[4], (unsigned long long)kFnoStatusRequire);
    else if (verdict == fno1i::kCandidate) {
        if (lists_are_short(a, ne.v1, ne.v2)) k = induced_kept(check_edge_lane(a, ne.v1, ne.v2));
        else l = 1;
    }
    keep[t] = k;
    is_long[t] = l;
}

__global__ __launch_bounds__(kBlock) void f1r_induced_waves_kernel(Groups g, const uint32_t* __restrict__ long_idx, const unsigned long long* __restrict__ n_long,
                                                                   Adj a, uint8_t* __restrict__ keep) {
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / 64, n_waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t n = *n_long;
    for (uint64_t k = wave; k < n; k += n_waves) {
        const uint32_t t = long_idx[k];
        hc_fno_edge ne;
        if (induced_of(g, a, t, &ne) != fno1i::kCandidate) continue;  // (wave-uniform: every lane computes the same pair)
        const double r = check_edge_wave(a, ne.v1, ne.v2, lane);
        if (lane == 0) keep[t] = induced_kept(r);
    }
}

__global__ __launch_bounds__(kBlock) void f1r_induced_build_kernel(Groups g, const uint32_t* __restrict__ idx, uint64_t n, Adj a, hc_fno_edge* __restrict__ out) {
    const uint64_t k = gid();
    if (k >= n) return;
    hc_fno_edge ne;
    if (induced_of(g, a, idx[k], &ne) != fno1i::kCandidate) return;  // (kept pairs are candidates)
    const uint4* src = reinterpret_cast<const uint4*>(&ne);
    uint4* dst = reinterpret_cast<uint4*>(out + k);
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

__global__ __launch_bounds__(kBlock) void f1r_cliques_kernel(const uint64_t* __restrict__ clique_off, uint64_t n_srs, unsigned long long* __restrict__ status) {
    const uint64_t i = gid();
    if (i >= n_srs) return;
    if (!(clique_off[i + 1] > clique_off[i])) atomicOr(&status[4], (unsigned long long)kFnoStatusRequire);  // get_sorted_clique asserts size() > 0
}

__global__ __launch_bounds__(kBlock) void f1r_subread_keys_kernel(const uint64_t* __restrict__ subread_off, const hc_fno_subread* __restrict__ subreads,
                                                                  uint64_t n_srs, uint64_t total, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
                                                                  unsigned long long* __restrict__ status) {
    const uint64_t e = gid();
    if (e >= total) return;
    const uint64_t sr = owner(subread_off, n_srs, e), node = subreads[e].node;
    if (node >> 32) atomicOr(&status[4], (unsigned long long)kFnoStatusRange);  // (no vertex of a graph on the device: the look-up would fail anyway)
    key[e] = sr << 32 | (node & 0xFFFFFFFFull);
    val[e] = (uint32_t)e;
}

__global__ __launch_bounds__(kBlock) void f1r_subread_gather_kernel(const hc_fno_subread* __restrict__ subreads, const uint32_t* __restrict__ val_sorted,
                                                                    uint64_t total, hc_fno_subread* __restrict__ out) {
    const uint64_t p = gid();
    if (p < total) out[p] = subreads[val_sorted[p]];
}

__global__ __launch_bounds__(kBlock) void f1r_line_heads_kernel(const uint64_t* __restrict__ len, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t i = gid();
    if (i > n) return;
    head[i] = i < n && len[i] != 0 ? 1u : 0u;
}

static_assert(sizeof(hc_line_rec) == 48, "a line record is three 16-byte words");
__global__ __launch_bounds__(kBlock) void f1r_line_records_kernel(const FnoRec* __restrict__ rec, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ len,
                                                                  const uint32_t* __restrict__ rank, uint64_t n, hc_line_rec* __restrict__ lines, uint64_t n_lines) {
    const uint64_t i = gid();
    if (i >= n || len[i] == 0) return;
    const uint64_t at = rank[i];
    if (at >= n_lines) return;  // (cannot happen: n_lines is the count of the heads)
    const FnoRec r = rec[perm[i]];
    uint4* dst = reinterpret_cast<uint4*>(lines + at);
    dst[0] = make_uint4((uint32_t)r.id1, (uint32_t)(r.id1 >> 32), (uint32_t)r.id2, (uint32_t)(r.id2 >> 32));
    dst[1] = make_uint4((uint32_t)r.pos1, (uint32_t)r.pos2, (uint32_t)r.perc, 0u);  // pos1 pos2 | perc1 perc2 (the text's "0")
    dst[2] = make_uint4((uint32_t)r.len1, (uint32_t)r.len2, (uint32_t)r.ord2 | (uint32_t)r.ori1 << 8 | (uint32_t)r.ori2 << 16 | (uint32_t)r.type1 << 24,
                        (uint32_t)r.type2);  // len1 len2 | ord ori1 ori2 type1 | type2 pad
}

}  // namespace

hipError_t convert(const hc_edge_rec* in, uint64_t n, hc_fno_edge* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(f1r_convert_kernel, grid_for(n), dim3(kBlock), 0, s, in, n, out);
    return hipGetLastError();
}
hipError_t group_pairs(const uint64_t* off, uint64_t n_groups, uint64_t* cnt, hipStream_t s) {
    hipLaunchKernelGGL(f1r_group_pairs_kernel, grid_for(n_groups + 1), dim3(kBlock), 0, s, off, n_groups, cnt);
    return hipGetLastError();
}
hipError_t nonedge_lanes(const hc_fno_edge* non, uint64_t n, const Adj& a, uint8_t* keep, uint8_t* is_long, unsigned long long* status, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(f1r_nonedge_lanes_kernel, grid_for(n), dim3(kBlock), 0, s, non, n, a, keep, is_long, status);
    return hipGetLastError();
}
hipError_t nonedge_waves(const hc_fno_edge* non, const uint32_t* long_idx, const unsigned long long* n_long, const Adj& a, uint8_t* keep, uint32_t n_cu,
                         hipStream_t s) {
    hipLaunchKernelGGL(f1r_nonedge_waves_kernel, dim3(n_cu * 4), dim3(kBlock), 0, s, non, long_idx, n_long, a, keep);
    return hipGetLastError();
}
hipError_t induced_lanes(const Groups& g, uint64_t n_pairs, const Adj& a, uint8_t* keep, uint8_t* is_long, unsigned long long* status, hipStream_t s) {
    if (!n_pairs) return hipSuccess;
    hipLaunchKernelGGL(f1r_induced_lanes_kernel, grid_for(n_pairs), dim3(kBlock), 0, s, g, n_pairs, a, keep, is_long, status);
    return hipGetLastError();
}
hipError_t induced_waves(const Groups& g, const uint32_t* long_idx, const unsigned long long* n_long, const Adj& a, uint8_t* keep, uint32_t n_cu,
                         hipStream_t s) {
    hipLaunchKernelGGL(f1r_induced_waves_kernel, dim3(n_cu * 4), dim3(kBlock), 0, s, g, long_idx, n_long, a, keep);
    return hipGetLastError();
}
hipError_t induced_build(const Groups& g, const uint32_t* idx, uint64_t n, const Adj& a, hc_fno_edge* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(f1r_induced_build_kernel, grid_for(n), dim3(kBlock), 0, s, g, idx, n, a, out);
    return hipGetLastError();
}
hipError_t cliques_check(const uint64_t* clique_off, uint64_t n_srs, unsigned long long* status, hipStream_t s) {
    if (!n_srs) return hipSuccess;
    hipLaunchKernelGGL(f1r_cliques_kernel, grid_for(n_srs), dim3(kBlock), 0, s, clique_off, n_srs, status);
    return hipGetLastError();
}
hipError_t subread_keys(const uint64_t* subread_off, const hc_fno_subread* subreads, uint64_t n_srs, uint64_t total, uint64_t* key, uint32_t* val,
                        unsigned long long* status, hipStream_t s) {
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(f1r_subread_keys_kernel, grid_for(total), dim3(kBlock), 0, s, subread_off, subreads, n_srs, total, key, val, status);
    return hipGetLastError();
}
hipError_t subread_gather(const hc_fno_subread* subreads, const uint32_t* val_sorted, uint64_t total, hc_fno_subread* out, hipStream_t s) {
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(f1r_subread_gather_kernel, grid_for(total), dim3(kBlock), 0, s, subreads, val_sorted, total, out);
    return hipGetLastError();
}
hipError_t line_heads(const uint64_t* len, uint64_t n, uint32_t* head, hipStream_t s) {
    hipLaunchKernelGGL(f1r_line_heads_kernel, grid_for(n + 1), dim3(kBlock), 0, s, len, n, head);
    return hipGetLastError();
}
hipError_t line_records(const FnoRec* rec, const uint32_t* perm, const uint64_t* len, const uint32_t* rank, uint64_t n, hc_line_rec* lines, uint64_t n_lines,
                        hipStream_t s) {
    if (!n || !n_lines) return hipSuccess;
    hipLaunchKernelGGL(f1r_line_records_kernel, grid_for(n), dim3(kBlock), 0, s, rec, perm, len, rank, n, lines, n_lines);
    return hipGetLastError();
}

}  // namespace fno1r
}  // namespace hc
