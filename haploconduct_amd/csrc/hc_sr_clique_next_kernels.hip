// hc_sr_clique_next_kernels.hip — the device side of hc_sr_clique_next (include/hcsr.h): what SRBuilder::cliquesToSuperreads does between
// the consensus of the cliques and find-next-overlaps (reference src/SRBuilder.cpp:981-1001, :1122-1233), on the arrays a clique merge
// returned.  Integer gathers, one lane per item: a clique vertex, a clique, a layout member, a surviving super-read, an index entry of a
// self-merged clique — never a loop over a clique, so that one clique of 10^4 vertices costs what 10^4 pairs cost.  A lane finds its
// clique by bisection (hc_sr_clique_next.h: clique_of_item, owner_of, find_vertex).  The vertices' half of the work is hc_sr_merge_next's own
// kernels (launch_vertices, launch_vertex_finish, launch_order with no pairs); the bytes are touched only by hc_sr_next_kernels.hip's
// check and gather.  No atomics: the marks are plain byte stores of 1, every other lane owns what it writes, and every place comes from
// an exclusive sum.
//
// cn_items_kernel        item j of clique_nodes -> clique << 32 | vertex, for the sort that puts every clique's vertices in ascending order
//                        (clique merge's step 1): the order `subreads` is in.
// cn_cliques_kernel      clique i -> slot i: the entry of its super-read (clique_entry) or a kind the check kernel refuses.
// cn_members_kernel      member m -> the clique whose FIRST layout it belongs to, where its vertex lies among the sorted keys, and how
//                        many index entries the vertex gives a self-merged clique.
// cn_mark_kernel         after the check: visited[member_vertex[m]] = 1 for every member of a surviving clique's first layout.
// cn_keys_kernel         after the check: the clique's term of the rank sum.
// cn_order_kernel        after the sum: a surviving clique's entry to its place in singles / trivials / pairs order, ids, kinds, srs,
//                        sr_clique, and the sizes of its row, of its subread list and of its index entries.
// cn_member_rows_kernel  after the sums of the sizes: a member's vertex to the plain row, or its index entries (vertex, index1),
//                        (vertex, index2 + overlap_pos) in the pre-order: descending member position, index1 first.
// cn_subreads_kernel     sorted item j -> its hc_fno_subread, index2 shifted after a self-merge.
// cn_merged_rows_kernel  after the stable sort of the index entries by (super-read, index): entry t -> its place in the row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr_clique_next.h"

namespace hc {
namespace cn {
namespace {

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ __launch_bounds__(256) void cn_items_kernel(In I, Work W) {
    const uint64_t j = gid();
    if (j >= I.n_items) return;
    W.key_in[j] = item_key(clique_of_item(I.clique_off, I.n_cliques, j), I.clique_nodes[j]);
}

__global__ __launch_bounds__(256) void cn_cliques_kernel(In I, Work W, mn::Slots S) {
    const uint64_t i = gid();
    if (i >= I.n_cliques) return;
    hc_sr_next_entry e;
    clique_entry(I, i, W.bad[i] != 0, e);
    S.entries[i] = e;
    S.overlap_pos[i] = -1;
}

__global__ __launch_bounds__(256) void cn_members_kernel(In I, Work W) {
    const uint64_t m = gid();
    if (m == 0) W.m_cnt[I.n_members] = 0;
    if (m >= I.n_members) return;
    const uint32_t o = owner_of(W.own, W.n_own, m);
    uint32_t item = kNone;
    if (o != kNone) {
        const uint64_t i = W.own[o].clique;
        item = find_vertex(W.key, I.clique_off[i], I.clique_off[i + 1], i, I.member_vertex[m]);
    }
    W.m_owner[m] = o;
    W.m_item[m] = item;
    W.m_cnt[m] = item != kNone ? member_items(I.subreads[item]) : 0;
}

__global__ __launch_bounds__(256) void cn_mark_kernel(In I, Work W, mn::Slots S) {
    const uint64_t m = gid();
    if (m >= I.n_members) return;
    const uint32_t o = W.m_owner[m];
    if (o == kNone || S.status[W.own[o].clique] != HC_SR_NEXT_KEPT) return;
    S.visited[I.member_vertex[m]] = 1;  // (an owner passed vertices_ok: inside the graph)
}

__global__ __launch_bounds__(256) void cn_keys_kernel(In I, mn::Slots S) {
    const uint64_t i = gid();
    if (i >= I.n_cliques) return;
    S.key[i] = S.status[i] != HC_SR_NEXT_KEPT ? 0ull : S.entries[i].kind == HC_SR_NEXT_SINGLE ? 1ull : 1ull << 32;
}

__global__ __launch_bounds__(256) void cn_order_kernel(In I, Work W, mn::Slots S, mn::Totals N, hc_sr_next_entry* __restrict__ out_entries,
                                                       uint32_t* __restrict__ out_status, uint64_t* __restrict__ out_cnt,
                                                       uint64_t* __restrict__ out_bytes, mn::Tables T) {
    const uint64_t i = gid();
    if (i == 0) {
        const uint32_t n_srs = N.n_singles + N.n_paired;
        T.clique_cnt[n_srs] = 0;
        W.sub_cnt[n_srs] = 0;
        W.pre_cnt[n_srs] = 0;
    }
    if (i >= I.n_cliques) return;
    const uint64_t r = S.rank[i];
    const uint32_t lo = (uint32_t)r, hi = (uint32_t)(r >> 32);
    const hc_sr_next_entry e = S.entries[i];
    const int32_t op = S.overlap_pos[i];
    T.pair_kind[i] = mn::pair_kind(e.kind, S.status[i], op >= 0);
    if (S.status[i] != HC_SR_NEXT_KEPT) {
        T.pair_new_id[i] = -1;
        W.sr_of[i] = kNone;
        return;
    }
    const bool single = e.kind == HC_SR_NEXT_SINGLE;
    const uint32_t pos = single ? lo : N.n_singles + N.n_trivials + hi, k = single ? lo : N.n_singles + hi;
    const hc_sr_layout L = I.layouts[I.first_layout[i]];
    const uint64_t n_index = W.m_off[L.first_member + L.n_members] - W.m_off[L.first_member];
    T.clique_cnt[k] = op >= 0 ? n_index : L.n_members;
    W.pre_cnt[k] = op >= 0 ? n_index : 0;
    W.sub_cnt[k] = I.clique_off[i + 1] - I.clique_off[i];
    W.sr_of[i] = k;
    T.sr_pair[k] = (uint32_t)i;
    hc_fno_read sr{};
    sr.id = pos;
    sr.len1 = e.len1;
    sr.len2 = single ? 0 : e.len2;
    sr.paired = single ? 0 : 1;
    T.srs[k] = sr;
    T.pair_new_id[i] = (int32_t)pos;
    out_entries[pos] = e;
    out_status[pos] = HC_SR_NEXT_KEPT;
    out_cnt[pos] = S.cnt[i];
    out_bytes[pos] = S.bytes[i];
}

__global__ __launch_bounds__(256) void cn_member_rows_kernel(In I, Work W, mn::Slots S, mn::Tables T) {
    const uint64_t m = gid();
    if (m >= I.n_members) return;
    const uint32_t o = W.m_owner[m];
    if (o == kNone) return;
    const Owner own = W.own[o];
    const uint32_t k = W.sr_of[own.clique];
    if (k == kNone) return;
    const uint32_t x = I.member_vertex[m];
    const int32_t op = S.overlap_pos[own.clique];
    if (op < 0) {  // get_sorted_clique(0) / (1), :853, :864
        T.clique_nodes[T.clique_off[k] + (m - own.first_member)] = x;
        return;
    }
    const uint32_t item = W.m_item[m];
    if (item == kNone) return;
    const hc_sr_subread_info s = I.subreads[item];
    const uint64_t at = W.pre_off[k] + (W.m_off[own.first_member + own.n_members] - W.m_off[m + 1]);  // the entries of the members behind m come first
    W.it_key_in[at] = index_key(k, s.index1);
    W.it_val_in[at] = x;
    if (s.index2 >= 0) {
        W.it_key_in[at + 1] = index_key(k, mn::shift_index2(s.index2, op));
        W.it_val_in[at + 1] = x;
    }
}

__global__ __launch_bounds__(256) void cn_subreads_kernel(In I, Work W, mn::Slots S, mn::Tables T) {
    const uint64_t j = gid();
    if (j >= I.n_items) return;
    const uint64_t key = W.key[j], i = key >> 32;
    const uint32_t k = W.sr_of[i];
    if (k == kNone) return;
    const hc_sr_subread_info s = I.subreads[j];  // (the sort keeps every clique's range: j is clique_off[i] + the vertex's rank)
    const int32_t op = S.overlap_pos[i];
    T.subreads[T.subread_off[k] + (j - I.clique_off[i])] =
        hc_fno_subread{(uint32_t)key, s.index1, op >= 0 ? mn::shift_index2(s.index2, op) : s.index2, s.startpos1, s.startpos2};
}

__global__ __launch_bounds__(256) void cn_merged_rows_kernel(Work W, uint64_t n_entries, mn::Tables T) {
    const uint64_t t = gid();
    if (t >= n_entries) return;
    const uint64_t k = W.it_key[t] >> 32;
    T.clique_nodes[T.clique_off[k] + (t - W.pre_off[k])] = W.it_val[t];
}

inline dim3 lanes(uint64_t n) { return dim3((uint32_t)((n + 255) / 256 ? (n + 255) / 256 : 1)); }  // (n < 2^32)

}  // namespace

hipError_t launch_items(In I, Work W, hipStream_t stream) {
    hipLaunchKernelGGL(cn_items_kernel, lanes(I.n_items), dim3(256), 0, stream, I, W);
    return hipGetLastError();
}
hipError_t launch_cliques(In I, Work W, mn::Slots S, hipStream_t stream) {
    hipLaunchKernelGGL(cn_cliques_kernel, lanes(I.n_cliques), dim3(256), 0, stream, I, W, S);
    return hipGetLastError();
}
hipError_t launch_members(In I, Work W, hipStream_t stream) {
    hipLaunchKernelGGL(cn_members_kernel, lanes(I.n_members), dim3(256), 0, stream, I, W);
    return hipGetLastError();
}
hipError_t launch_mark(In I, Work W, mn::Slots S, hipStream_t stream) {
    hipLaunchKernelGGL(cn_mark_kernel, lanes(I.n_members), dim3(256), 0, stream, I, W, S);
    return hipGetLastError();
}
hipError_t launch_keys(In I, mn::Slots S, hipStream_t stream) {
    hipLaunchKernelGGL(cn_keys_kernel, lanes(I.n_cliques), dim3(256), 0, stream, I, S);
    return hipGetLastError();
}
hipError_t launch_order(In I, Work W, mn::Slots S, mn::Totals N, hc_sr_next_entry* out_entries, uint32_t* out_status, uint64_t* out_cnt,
                        uint64_t* out_bytes, mn::Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(cn_order_kernel, lanes(I.n_cliques), dim3(256), 0, stream, I, W, S, N, out_entries, out_status, out_cnt, out_bytes, T);
    return hipGetLastError();
}
hipError_t launch_member_rows(In I, Work W, mn::Slots S, mn::Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(cn_member_rows_kernel, lanes(I.n_members), dim3(256), 0, stream, I, W, S, T);
    return hipGetLastError();
}
hipError_t launch_subreads(In I, Work W, mn::Slots S, mn::Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(cn_subreads_kernel, lanes(I.n_items), dim3(256), 0, stream, I, W, S, T);
    return hipGetLastError();
}
hipError_t launch_merged_rows(Work W, uint64_t n_entries, mn::Tables T, hipStream_t stream) {
    hipLaunchKernelGGL(cn_merged_rows_kernel, lanes(n_entries), dim3(256), 0, stream, W, n_entries, T);
    return hipGetLastError();
}

}  // namespace cn
}  // namespace hc
