// hc_sr_merge_next_kernels.hip — the device side of hc_sr_merge_next (include/hcsr.h): what SRBuilder::mergeAlongEdges does between the
// consensus of the picked edges and find-next-overlaps (reference src/SRBuilder.cpp:981-1001, :1260-1380), on the arrays an edge merge
// returned.  Integer gathers, one lane per pair / vertex / super-read, bound by latency like hc_sr_edge_kernels.hip; the bytes are
// touched only by hc_sr_next_kernels.hip's check and gather, which run between these.  No atomics: every lane owns its slot, and the
// places in the final order come from one exclusive sum.
//
// mn_pairs_kernel      pair i -> slot i: the entry of its super-read (hc_sr_merge_next.h: pair_entry) or a kind the check kernel refuses.
// mn_rewrite_kernel    a pair merge_self_overlap merged: its entry becomes the single-end read the kept form appended.
// mn_mark_kernel       after the check: visited[v] = visited[w] = 1 for a pair that survived (plain byte stores of the same value: two
//                      pairs naming one vertex cannot disagree), and the pair's term of the rank sum.
// mn_vertices_kernel   vertex v -> slot n_pairs + v: a trivial entry when nobody marked it.
// mn_vertex_finish_kernel  after the check again: the inclusion and tip tests behind hc_sr_next's two (:1286-1311), the final mark, the
//                      vertex's term of the rank sum.
// mn_order_kernel      after the sum: every survivor's entry to its place in singles / trivials / pairs order with what the gather's own
//                      sums need, the ids, the kinds, `nodes`, the tips list and, per super-read, srs / sr_pair / the clique's size (the
//                      pair kernel's count of members, or the count of a self-merged pair's index entries).
// mn_tables_kernel     after the sum of the sizes: clique_nodes and subreads, the self-merge shift and the four-element ordering in
//                      registers (hc_sr_merge_next.h: sr_tables).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr_merge_next.h"

namespace hc {
namespace mn {
namespace {

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ __launch_bounds__(256) void mn_pairs_kernel(In I, Slots S) {
    const uint64_t i = gid();
    if (i >= I.n_pairs) return;
    hc_sr_next_entry e;
    uint32_t nc;
    pair_entry(I, i, e, nc);
    S.entries[i] = e;
    S.n_clique[i] = (uint8_t)nc;
    S.overlap_pos[i] = -1;
}

__global__ __launch_bounds__(256) void mn_rewrite_kernel(const Rewrite* __restrict__ rw, uint64_t n, uint64_t n_pairs, Slots S) {
    const uint64_t k = gid();
    if (k >= n) return;
    const Rewrite r = rw[k];
    if (r.pair >= n_pairs) return;
    S.entries[r.pair] = hc_sr_next_entry{r.off, 0, r.len, 0, 0, HC_SR_NEXT_SINGLE, HC_SR_SRC_CONSENSUS, HC_SR_SRC_CONSENSUS, 0};
    S.overlap_pos[r.pair] = r.overlap_pos;
}

__global__ __launch_bounds__(256) void mn_mark_kernel(In I, Slots S) {
    const uint64_t i = gid();
    if (i >= I.n_pairs) return;
    const bool kept = S.status[i] == HC_SR_NEXT_KEPT;  // (kept: pair_entry found both vertices inside the graph)
    S.key[i] = !kept ? 0ull : S.entries[i].kind == HC_SR_NEXT_SINGLE ? 1ull : 1ull << 32;
    if (!kept) return;
    S.visited[I.pairs[2 * i]] = 1;
    S.visited[I.pairs[2 * i + 1]] = 1;
}

__device__ inline uint32_t n_mates_of(const SrNextSources& src, uint32_t read) {
    return read < src.n_reads ? src.raw_first[read + 1] - src.raw_first[read] : 0u;
}

__global__ __launch_bounds__(256) void mn_vertices_kernel(In I, Slots S, SrNextSources src) {
    const uint64_t v = gid();
    if (v >= I.n_vertices) return;
    const uint32_t read = I.vertex_read[v];
    hc_sr_next_entry e{0, 0, 0, 0, read, kNoEntry, 0, 0, (uint8_t)(I.vertex_fwd[v] ? 0 : 1)};
    if (!S.visited[v]) e.kind = n_mates_of(src, read) == 2 ? HC_SR_NEXT_TRIVIAL_PAIRED : HC_SR_NEXT_TRIVIAL;  // (no such read: the check refuses it)
    S.entries[I.n_pairs + v] = e;
}

__global__ __launch_bounds__(256) void mn_vertex_finish_kernel(In I, Slots S, uint32_t ignore_inclusions, uint32_t store_tips, Tables T) {
    const uint64_t v = gid();
    if (v >= I.n_vertices) return;
    const uint64_t j = I.n_pairs + v;
    const uint32_t read = I.vertex_read[v];
    const bool tip = I.tip_reads && read < I.n_reads && I.tip_reads[read];
    const uint32_t state = vertex_state(S.visited[v] != 0, S.status[j], ignore_inclusions != 0, I.inclusions && I.inclusions[v], store_tips != 0, tip);
    const bool held = state == HC_SR_MN_V_INCLUSION || state == HC_SR_MN_V_TIP;
    if (held) {  // (it passed the tests of a trivial: off the entry list all the same)
        S.status[j] = kHeld;
        S.cnt[j] = 0;
        S.bytes[j] = 0;
    }
    T.vertex_state[v] = state;
    S.visited[v] = state != HC_SR_MN_V_TRIVIAL;  // :1287, :1293, :1301, :1308
    S.key[j] = state == HC_SR_MN_V_TRIVIAL ? 1ull : held ? 1ull << 32 : 0ull;
    if (v == 0) S.key[I.n_pairs + I.n_vertices] = 0;
}

__global__ __launch_bounds__(256) void mn_order_kernel(In I, Slots S, Totals N, SrNextSources src, hc_sr_next_entry* __restrict__ out_entries,
                                                       uint32_t* __restrict__ out_status, uint64_t* __restrict__ out_cnt,
                                                       uint64_t* __restrict__ out_bytes, Tables T) {
    const uint64_t j = gid(), n_slots = I.n_pairs + I.n_vertices;
    const uint32_t n_kept = N.n_singles + N.n_trivials + N.n_paired;
    if (j == 0) {
        out_cnt[n_kept] = 0;
        out_bytes[n_kept] = 0;
        T.clique_cnt[N.n_singles + N.n_paired] = 0;
    }
    if (j >= n_slots) return;
    const uint64_t r = S.rank[j];
    const uint32_t lo = (uint32_t)r, hi = (uint32_t)(r >> 32);
    const bool kept = S.status[j] == HC_SR_NEXT_KEPT;
    const hc_sr_next_entry e = S.entries[j];
    uint32_t pos = 0;
    if (j < I.n_pairs) {
        const int32_t op = S.overlap_pos[j];
        T.pair_kind[j] = pair_kind(e.kind, S.status[j], op >= 0);
        if (kept) {
            const bool single = e.kind == HC_SR_NEXT_SINGLE;
            pos = single ? lo : N.n_singles + N.n_trivials + hi;
            const uint32_t k = single ? lo : N.n_singles + hi;
            T.clique_cnt[k] = op >= 0 ? merged_clique_size(I.subreads[2 * j], I.subreads[2 * j + 1], op) : S.n_clique[j];
            T.sr_pair[k] = (uint32_t)j;
            hc_fno_read sr{};
            sr.id = pos;
            sr.len1 = e.len1;
            sr.len2 = single ? 0 : e.len2;
            sr.paired = single ? 0 : 1;
            T.srs[k] = sr;
        }
        T.pair_new_id[j] = kept ? (int32_t)pos : -1;
    } else {
        const uint64_t v = j - I.n_pairs;
        pos = lo;  // the singles, then the trivials before v
        const uint32_t read = I.vertex_read[v], nm = n_mates_of(src, read);
        hc_fno_read nd{};
        if (nm) {
            const uint32_t q = src.raw_first[read];
            nd.len1 = (uint32_t)(src.raw_off[q + 1] - src.raw_off[q]);
            nd.len2 = nm == 2 ? (uint32_t)(src.raw_off[q + 2] - src.raw_off[q + 1]) : 0;
            nd.paired = nm == 2;
        }
        nd.id = kept ? pos : 0;
        nd.visited = S.visited[v];
        nd.orientation = I.vertex_fwd[v] ? 1 : 0;
        T.nodes[v] = nd;
        if (S.status[j] == kHeld) T.tips[hi - N.n_paired] = (uint32_t)v;
    }
    if (!kept) return;
    out_entries[pos] = e;
    out_status[pos] = HC_SR_NEXT_KEPT;
    out_cnt[pos] = S.cnt[j];
    out_bytes[pos] = S.bytes[j];
}

__global__ __launch_bounds__(256) void mn_tables_kernel(In I, Slots S, uint64_t n_srs, Tables T) {
    const uint64_t k = gid();
    if (k == 0) T.subread_off[n_srs] = 2 * n_srs;
    if (k >= n_srs) return;
    const uint32_t i = T.sr_pair[k];
    uint64_t clique[4];
    hc_fno_subread sub[2];
    const uint32_t n = sr_tables(I, i, S.overlap_pos[i], clique, sub);
    const uint64_t at = T.clique_off[k];
    for (uint32_t a = 0; a < n; a++) T.clique_nodes[at + a] = clique[a];
    T.subread_off[k] = 2 * k;
    T.subreads[2 * k] = sub[0];
    T.subreads[2 * k + 1] = sub[1];
}

inline dim3 lanes(uint64_t n) { return dim3((uint32_t)((n + 255) / 256 ? (n + 255) / 256 : 1)); }  // (n < 2^31)

}  // namespace

hipError_t launch_pairs(In I, Slots S, hipStream_t stream) {
    hipLaunchKernelGGL(mn_pairs_kernel, lanes(I.n_pairs), dim3(256), 0, stream, I, S);
    return hipGetLastError();
}
hipError_t launch_rewrite(const Rewrite* rw, uint64_t n, uint64_t n_pairs, Slots S, hipStream_t stream) {
    hipLaunchKernelGGL(mn_rewrite_kernel, lanes(n), dim3(256), 0, stream, rw, n, n_pairs, S);
    return hipGetLastError();
}
hipError_t launch_mark(In I, Slots S, hipStream_t stream) {
    hipLaunchKernelGGL(mn_mark_kernel, lanes(I.n_pairs), dim3(256), 0, stream, I, S);
    return hipGetLastError();
}
hipError_t launch_vertices(In I, Slots S, SrNextSources src, hipStream_t stream) {
    hipLaunchKernelGGL(mn_vertices_kernel, lanes(I.n_vertices), dim3(256), 0, stream, I, S, src);
    return hipGetLastError();
}
hipError_t launch_vertex_finish(In I, Slots S, uint32_t ignore_inclusions, uint32_t store_tips, Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(mn_vertex_finish_kernel, lanes(I.n_vertices), dim3(256), 0, stream, I, S, ignore_inclusions, store_tips, T);
    return hipGetLastError();
}
hipError_t launch_order(In I, Slots S, Totals N, SrNextSources src, hc_sr_next_entry* out_entries, uint32_t* out_status, uint64_t* out_cnt,
                        uint64_t* out_bytes, Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(mn_order_kernel, lanes(I.n_pairs + I.n_vertices), dim3(256), 0, stream, I, S, N, src, out_entries, out_status, out_cnt, out_bytes,
                       T);
    return hipGetLastError();
}
hipError_t launch_tables(In I, Slots S, uint64_t n_srs, Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(mn_tables_kernel, lanes(n_srs), dim3(256), 0, stream, I, S, n_srs, T);
    return hipGetLastError();
}

}  // namespace mn
}  // namespace hc
