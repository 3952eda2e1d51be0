// hc_sr_edge_kernels.hip — the edge merge on the device graph (include/hcsr.h: hc_graph_merge_pairs, hc_sr_edge_merge):
// what SRBuilder::mergeAlongEdges (reference src/SRBuilder.cpp:1238-1253) does between the cleaned graph and consensus().
//
// sr_edge_target_kernel writes the target column of the out-records as packed 32-bit ids, for the host's walk of
// OverlapGraph::getEdgesForMerging (src/GraphAlgos.cpp:112-148).
// sr_edge_layout_kernel (one lane per pair) does constructSuperread's ordering, type and base choice (src/SRBuilder.cpp:658-698) and
// sort_vertices (:33-285) for a clique of two.  getEdgeInfo (src/OverlapGraph.cpp:263-282) is a scan in list order: a lane walks a list
// of fewer than 64 records, the wave walks a longer one 64 records at a time and stops at the first chunk with a hit (the split of
// hc_trans_kernels.hip: k_list_sum; hc_sr_lay.h: find_first, shared with the clique kernels as is the per-node part of the loop).  The list the reference builds by insertion (:198-222) has at most three entries; its order is
// (position ascending, insertion number descending), which three comparisons give.  Pairedness and lengths come from the store's read
// descriptors; no symbol is read.  A pair writes into slots of its own; sr_edge_compact_kernel packs layouts and members behind two
// exclusive sums.  sr_edge_subread_kernel is calcSubreadInfo (:536-595), one lane per pair, behind the consensus.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr.h"
#include "hc_sr_lay.h"

namespace hc {
namespace {

using namespace srlay;  // find_first, FoundEdge, base_member, lay_node, sub_place

__global__ __launch_bounds__(256) void sr_edge_target_kernel(const hc_edge_rec* __restrict__ E, uint64_t n, uint32_t* __restrict__ tgt) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) tgt[k] = (uint32_t)E[k].v2;
}

struct Entry {
    int64_t pos;
    uint32_t len, ins;  // ins: the insertion number (0 = the base)
    hc_sr_member m;
    uint8_t who;
};

// an entry inserted later goes in front of the first whose position is not smaller (:198-222)
__device__ inline bool before(const Entry& x, const Entry& y) { return x.pos < y.pos || (x.pos == y.pos && x.ins > y.ins); }

// sort_vertices for {base, node} with the record found: HC_SR_EDGE_*; on OK the members (positions shifted), who and total_len
__device__ uint32_t lay_one(const StoreView& st, char type, uint32_t base_ID, const ReadDesc& bd, bool base_fwd, bool node_fwd, uint8_t base_who,
                            const FoundEdge& e, hc_sr_member* out, uint8_t* who, uint32_t* n_out, int32_t* total_out) {
    Entry en[3];
    en[0].pos = 0;
    en[0].ins = 0;
    en[0].who = base_who;
    en[0].m = base_member(type, base_ID, base_fwd);  // :47-76
    en[0].len = en[0].m.seq == 2 ? bd.len2 : bd.len1;
    const int64_t base_len = en[0].len;
    NodeLay nl;
    const uint32_t st_node = lay_node(st, type, base_ID, base_len, node_fwd, e, nl);  // :101-238, shared with the clique kernels
    if (st_node != HC_SR_EDGE_OK) return st_node;
    uint32_t n = 1;
    for (uint32_t k = 0; k < nl.n; k++) {
        Entry c;
        c.who = base_who ^ 1;
        c.m = nl.m[k];
        c.pos = nl.pos[k];
        c.len = nl.len[k];
        c.ins = n;
        en[n++] = c;
    }
    const int64_t len1 = nl.len1, len2 = nl.len2;
    const int64_t total_len = base_len + max(len1, (int64_t)0) + max(len2, (int64_t)0);  // :239-244
    if (total_len > INT32_MAX) return HC_SR_EDGE_BAD_GEOMETRY;
    // list order: (position ascending, insertion number descending)
    if (before(en[1], en[0])) {
        const Entry t = en[0];
        en[0] = en[1];
        en[1] = t;
    }
    if (n == 3) {
        if (before(en[2], en[1])) {
            const Entry t = en[1];
            en[1] = en[2];
            en[2] = t;
        }
        if (before(en[1], en[0])) {
            const Entry t = en[0];
            en[0] = en[1];
            en[1] = t;
        }
    }
    if (!(total_len > en[n - 1].pos)) return HC_SR_EDGE_BAD_GEOMETRY;  // :246
    const int64_t mn = en[0].pos;  // :248-252 (the base stands at 0, so min <= 0 and the first entry ends at 0)
    bool ok = (int64_t)en[0].len <= total_len;  // :259
    for (uint32_t i = 0; i < n; i++) {
        const int64_t p = en[i].pos - (mn < 0 ? mn : 0);
        if (i && p + (int64_t)en[i].len > total_len) ok = false;  // :281 (p >= 0 and ascending by construction: :263-264)
        en[i].m.pos = (int32_t)p;
    }
    if (!ok || en[0].m.pos != 0) return HC_SR_EDGE_BAD_GEOMETRY;
    for (uint32_t i = 0; i < n; i++) {
        out[i] = en[i].m;
        who[i] = en[i].who;
    }
    *n_out = n;
    *total_out = (int32_t)total_len;
    return HC_SR_EDGE_OK;
}

__global__ __launch_bounds__(256) void sr_edge_layout_kernel(StoreView st, const hc_edge_rec* __restrict__ E, const unsigned long long* __restrict__ out_off,
                                                             uint32_t V, const uint32_t* __restrict__ pairs, uint64_t n_pairs,
                                                             const uint32_t* __restrict__ vertex_read, const uint8_t* __restrict__ vertex_fwd,
                                                             SrEdgeSlots S) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    // (no lane leaves before the scans: the wave takes the long lists together)
    const bool in_range = i < n_pairs;
    uint32_t va = 0, vb = 0, ra = 0, rb = 0;
    bool valid = false;
    if (in_range) {
        const uint32_t v = pairs[2 * i], w = pairs[2 * i + 1];
        va = min(v, w);  // :658
        vb = max(v, w);
        valid = vb < V && va != vb;
        if (valid) {
            ra = vertex_read[va];
            rb = vertex_read[vb];
            valid = ra < st.n_reads && rb < st.n_reads;
        }
    }
    ReadDesc da{}, db{};
    char type = 'p';
    uint32_t base = va, node = vb;
    if (valid) {
        da = st.reads[ra];
        db = st.reads[rb];
        if (!(da.flags & kReadPaired)) type = 's';  // :669-679: the first single-end read in sorted order
        else if (!(db.flags & kReadPaired)) {
            type = 's';
            base = vb;
            node = va;
        }
    }
    // getEdgeInfo(base, node): base -> node first, then node -> base
    uint32_t a = 0, b = 0;
    if (valid) {
        a = (uint32_t)out_off[base];
        b = (uint32_t)out_off[base + 1];
    }
    uint32_t k = find_first(E, a, b, node, lane);
    a = b = 0;
    if (valid && k == kNone) {
        a = (uint32_t)out_off[node];
        b = (uint32_t)out_off[node + 1];
    }
    const uint32_t k2 = find_first(E, a, b, base, lane);
    if (k == kNone) k = k2;
    if (i > n_pairs) return;
    if (i == n_pairs) {  // the scans' last entries
        S.lay_cnt[i] = 0;
        S.mem_cnt[i] = 0;
        return;
    }
    uint32_t status = HC_SR_EDGE_BAD_VERTEX, n_lay = 0, n_mem = 0;
    if (valid) {
        status = HC_SR_EDGE_NO_EDGE;
        if (k != kNone) {
            const hc_edge_rec& r = E[k];
            const FoundEdge e{r.read1, r.read2, r.pos1, r.pos2, r.ord};
            const bool base_is_a = base == va;
            const uint32_t base_ID = base_is_a ? ra : rb;
            const ReadDesc& bd = base_is_a ? da : db;
            const bool base_fwd = vertex_fwd[base] != 0, node_fwd = vertex_fwd[node] != 0;
            hc_sr_member* m = S.members + 6 * i;
            uint8_t* who = S.who + 6 * i;
            hc_sr_layout* L = S.layouts + 2 * i;
            uint32_t n0 = 0, n1 = 0;
            int32_t t0 = 0, t1 = 0;
            status = lay_one(st, type == 'p' ? 'l' : 's', base_ID, bd, base_fwd, node_fwd, base_is_a ? 0 : 1, e, m, who, &n0, &t0);
            if (status == HC_SR_EDGE_OK && type == 'p') status = lay_one(st, 'r', base_ID, bd, base_fwd, node_fwd, 0, e, m + 3, who + 3, &n1, &t1);
            if (status == HC_SR_EDGE_OK) {
                n_lay = type == 'p' ? 2 : 1;
                n_mem = n0 + n1;
                L[0].first_member = 0;
                L[0].n_members = n0;
                L[0].total_len = t0;
                L[1].first_member = 0;
                L[1].n_members = n1;
                L[1].total_len = t1;
            }
        }
    }
    S.status[i] = status;
    S.lay_cnt[i] = n_lay;
    S.mem_cnt[i] = n_mem;
}

__global__ __launch_bounds__(256) void sr_edge_compact_kernel(SrEdgeSlots S, uint64_t n_pairs, const uint64_t* __restrict__ first_layout,
                                                              const uint64_t* __restrict__ mem_off, hc_sr_layout* __restrict__ layouts,
                                                              hc_sr_member* __restrict__ members) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const uint32_t n_lay = (uint32_t)S.lay_cnt[i];
    uint64_t l = first_layout[i], m = mem_off[i];
    for (uint32_t k = 0; k < n_lay; k++) {
        hc_sr_layout L = S.layouts[2 * i + k];
        L.first_member = m;
        layouts[l++] = L;
        for (uint32_t j = 0; j < L.n_members; j++) members[m++] = S.members[6 * i + 3 * k + j];
    }
}

__global__ __launch_bounds__(256) void sr_edge_subread_kernel(SrEdgeSlots S, uint64_t n_pairs, const uint64_t* __restrict__ first_layout,
                                                              const SrLayoutInfo* __restrict__ info, hc_sr_subread_info* __restrict__ subreads) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    hc_sr_subread_info s[2] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
    const uint32_t n_lay = (uint32_t)S.lay_cnt[i];
    if (n_lay) {
        const uint64_t l0 = first_layout[i];
        const int32_t trim_pos1 = info[l0].ret, trim_pos2 = n_lay == 2 ? info[l0 + 1].ret : -1;
        bool present[2] = {false, false};
        const uint32_t n0 = S.layouts[2 * i].n_members;
        for (uint32_t j = 0; j < n0; j++) {  // :541-574
            const uint32_t w = S.who[6 * i + j] & 1u;
            const int32_t pos = S.members[6 * i + j].pos;
            if (present[w]) sub_place(trim_pos1, pos, s[w].index2, s[w].startpos2);
            else {
                sub_place(trim_pos1, pos, s[w].index1, s[w].startpos1);
                s[w].index2 = -1;
                s[w].startpos2 = -1;
                present[w] = true;
            }
        }
        if (trim_pos2 >= 0) {  // :575-593
            const uint32_t n1 = S.layouts[2 * i + 1].n_members;
            for (uint32_t j = 0; j < n1; j++) {
                const uint32_t w = S.who[6 * i + 3 + j] & 1u;
                sub_place(trim_pos2, S.members[6 * i + 3 + j].pos, s[w].index2, s[w].startpos2);
            }
        }
    }
    subreads[2 * i] = s[0];
    subreads[2 * i + 1] = s[1];
}

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t sr_edge_launch_targets(const hc_edge_rec* edges, uint64_t n_edges, uint32_t* targets, hipStream_t s) {
    if (n_edges == 0) return hipSuccess;
    hipLaunchKernelGGL(sr_edge_target_kernel, grid_for(n_edges), dim3(256), 0, s, edges, n_edges, targets);
    return hipGetLastError();
}

hipError_t sr_edge_launch_layouts(const StoreView& st, const hc_edge_rec* edges, const unsigned long long* out_off, uint64_t n_vertices,
                                  const uint32_t* pairs, uint64_t n_pairs, const uint32_t* vertex_read, const uint8_t* vertex_fwd, SrEdgeSlots slots,
                                  hipStream_t s) {
    hipLaunchKernelGGL(sr_edge_layout_kernel, grid_for(n_pairs + 1), dim3(256), 0, s, st, edges, out_off, (uint32_t)n_vertices, pairs, n_pairs,
                       vertex_read, vertex_fwd, slots);
    return hipGetLastError();
}

hipError_t sr_edge_launch_compact(SrEdgeSlots slots, uint64_t n_pairs, const uint64_t* first_layout, const uint64_t* mem_off, hc_sr_layout* layouts,
                                  hc_sr_member* members, hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(sr_edge_compact_kernel, grid_for(n_pairs), dim3(256), 0, s, slots, n_pairs, first_layout, mem_off, layouts, members);
    return hipGetLastError();
}

hipError_t sr_edge_launch_subreads(SrEdgeSlots slots, uint64_t n_pairs, const uint64_t* first_layout, const SrLayoutInfo* info,
                                   hc_sr_subread_info* subreads, hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(sr_edge_subread_kernel, grid_for(n_pairs), dim3(256), 0, s, slots, n_pairs, first_layout, info, subreads);
    return hipGetLastError();
}

}  // namespace hc
