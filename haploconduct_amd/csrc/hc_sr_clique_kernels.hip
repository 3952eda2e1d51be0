// hc_sr_clique_kernels.hip — constructSuperread for cliques of any size on the device graph (include/hcsr.h: hc_sr_clique_merge; reference
// src/SRBuilder.cpp:654-748).  A fixed number of launches whatever the clique sizes, no per-clique sorting code: every ordering is one
// stable hc::prims radix sort over all cliques' items (hc_api_sr_clique.cpp runs them between these kernels).
//   keys       item t of the call -> clique << 32 | vertex; sorted, a clique's run is its vertices ascending (:658)
//   precheck   one lane per item: the range checks, repeats by neighbour comparison, atomicMin of the first single-end rank (:669-679)
//   bases      one lane per clique: type, base, the length of the base's out-list
//   hits       one lane per record of the bases' lists (count / scan / expand): bisects the record's target in the clique's run and does
//              atomicMin of the LIST POSITION into the vertex's slot — the first base -> node record in list order (getEdgeInfo,
//              src/OverlapGraph.cpp:263-282), the base's list read once per clique
//   nodes      one lane per item: a vertex without a hit scans its own list for the base (find_first); the per-node part of the loop
//              (hc_sr_lay.h: lay_node, shared with the pair kernel); l_ext / r_ext by atomicMax from 0 (:239-240)
//   entries    one lane per item: a clique's entries in DESCENDING insertion order, so that one stable sort by (layout, biased position)
//              is the list order — position ascending, insertion number descending (:198-222)
//   geometry   one lane per entry: the shift by -min and the asserts of :246, :259, :264, :281 in 64-bit integers; the full lists
//   filter     one wave per layout of a clique larger than 3 * min_clique_size, on the entries sorted once more by (layout, endpos):
//              the group rule of host/SrCliqueFilter.h
//   status, compact, consensus_input, subreads: the verdict per clique, the packed outputs, the USED members for sr_consensus_run, and
//              calcSubreadInfo (:536-595) one lane per item behind the consensus.
// Every pass is an integer gather bound by latency; no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr.h"
#include "hc_sr_lay.h"
#include "host/SrCliqueFilter.h"

namespace hc {
namespace {

using namespace srlay;

constexpr unsigned long long kNoFail = ~0ull;

// the c with off[c] <= x < off[c + 1]; off[0] == 0, off ascends (equal neighbours: an empty range), x < off[n]
__device__ inline uint64_t owner(const uint64_t* __restrict__ off, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void sr_clique_key_kernel(SrCliqueView W, const uint32_t* __restrict__ nodes, uint64_t* __restrict__ key_in) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W.N) return;
    key_in[t] = (owner(W.off, W.C, t) << 32) | nodes[t];
}

__global__ __launch_bounds__(256) void sr_clique_init_kernel(SrCliqueView W) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W.C) return;
    const uint64_t sz = W.off[c + 1] - W.off[c];
    W.failkey[c] = sz < 2 ? (unsigned long long)HC_SR_CLIQUE_TOO_SMALL : kNoFail;  // :656
    W.base_rank[c] = kNone;
    W.geom[c] = 0;
    for (int k = 0; k < 4; k++) W.ext[4 * c + k] = 0;
}

__global__ __launch_bounds__(256) void sr_clique_precheck_kernel(StoreView st, SrCliqueView W) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= W.N) return;
    const uint64_t key = W.key[j], c = key >> 32;
    const uint32_t v = (uint32_t)key;
    const uint64_t r = j - W.off[c], sz = W.off[c + 1] - W.off[c];
    uint32_t status = HC_SR_EDGE_OK;
    uint32_t read = 0;
    if (v >= W.V) status = HC_SR_EDGE_BAD_VERTEX;
    else {
        read = W.vread[v];
        if (read >= st.n_reads) status = HC_SR_EDGE_BAD_VERTEX;
        else if (r && W.key[j - 1] == key) status = sz == 2 ? HC_SR_EDGE_BAD_VERTEX : HC_SR_CLIQUE_REPEATED_VERTEX;
    }
    if (status != HC_SR_EDGE_OK) atomicMin(&W.failkey[c], (unsigned long long)(r << 8 | status));
    else if (!(st.reads[read].flags & kReadPaired)) atomicMin(&W.base_rank[c], (uint32_t)r);  // :672-679
}

__global__ __launch_bounds__(256) void sr_clique_base_kernel(SrCliqueView W) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > W.C) return;
    if (c == W.C) {  // the scans' last entries
        W.deg[c] = 0;
        W.lay0[c] = 0;
        return;
    }
    const bool ok = W.failkey[c] == kNoFail;
    uint32_t br = W.base_rank[c];
    const uint8_t type = br == kNone ? 'p' : 's';
    if (br == kNone) br = 0;
    W.base_rank[c] = br;
    W.type[c] = type;
    uint64_t deg = 0;
    if (ok) {
        const uint32_t vb = (uint32_t)W.key[W.off[c] + br];
        deg = W.out_off[vb + 1] - W.out_off[vb];
    }
    W.deg[c] = deg;
    W.lay0[c] = ok ? (type == 'p' ? 2 : 1) : 0;
}

__global__ __launch_bounds__(256) void sr_clique_hit_kernel(SrCliqueView W, uint64_t n_records) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_records) return;
    const uint64_t c = owner(W.rec_off, W.C, t);
    const uint64_t a = W.off[c], b = W.off[c + 1];
    const uint32_t vb = (uint32_t)W.key[a + W.base_rank[c]];
    const uint64_t k = W.out_off[vb] + (t - W.rec_off[c]);
    const uint64_t target = W.E[k].v2;
    if (target >> 32) return;
    const uint64_t want = c << 32 | target;
    uint64_t lo = a, hi = b;  // the first j in [a, b) with key[j] >= want
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (W.key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    if (lo < b && W.key[lo] == want) atomicMin(&W.hit[lo], (uint32_t)k);
}

__device__ inline void put(SrCliqueSlot& S, uint32_t at, const NodeLay& nl, uint32_t from) {
    S.pos[at] = nl.pos[from];
    S.len[at] = nl.len[from];
    S.m[at] = nl.m[from];
}

__global__ __launch_bounds__(256) void sr_clique_node_kernel(StoreView st, SrCliqueView W) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    // (no lane leaves before the scan: the wave takes the long lists together)
    const bool in_range = j < W.N;
    uint64_t c = 0, jb = 0;
    uint32_t v = 0, vb = 0, k = kNone, a = 0, b = 0;
    bool ok = false;
    if (in_range) {
        const uint64_t key = W.key[j];
        c = key >> 32;
        v = (uint32_t)key;
        ok = W.lay0[c] != 0;  // (the range checks' verdict; failkey changes under this kernel)
        if (ok) {
            jb = W.off[c] + W.base_rank[c];
            vb = (uint32_t)W.key[jb];
            if (j != jb) {
                k = W.hit[j];
                if (k == kNone) {  // node -> base, src/OverlapGraph.cpp:272-279
                    a = (uint32_t)W.out_off[v];
                    b = (uint32_t)W.out_off[v + 1];
                }
            }
        }
    }
    const uint32_t k2 = find_first(W.E, a, b, vb, lane);
    if (k == kNone) k = k2;
    if (j > W.N) return;
    if (j == W.N) {
        W.ecnt[j] = 0;
        return;
    }
    if (!ok) {
        W.ecnt[j] = 0;
        return;
    }
    const uint8_t type = W.type[c];
    const uint32_t base_ID = W.vread[vb];
    const ReadDesc bd = st.reads[base_ID];
    const bool base_fwd = W.vfwd[vb] != 0;
    SrCliqueSlot S{};
    const hc_sr_member b0 = base_member(type == 'p' ? 'l' : 's', base_ID, base_fwd), b1 = base_member('r', base_ID, base_fwd);
    const int64_t base_len0 = b0.seq == 2 ? bd.len2 : bd.len1, base_len1 = b1.seq == 2 ? bd.len2 : bd.len1;
    S.n = type == 'p' ? 2 : 1;
    if (j == jb) {
        S.m[0] = b0;
        S.len[0] = (uint32_t)base_len0;
        if (type == 'p') {
            S.m[1] = b1;
            S.len[1] = (uint32_t)base_len1;
        }
    } else {
        uint32_t status = HC_SR_EDGE_NO_EDGE;
        if (k != kNone) {
            const hc_edge_rec& r = W.E[k];
            const FoundEdge e{r.read1, r.read2, r.pos1, r.pos2, r.ord};
            const bool node_fwd = W.vfwd[v] != 0;
            NodeLay nl;
            status = lay_node(st, type == 'p' ? 'l' : 's', base_ID, base_len0, node_fwd, e, nl);
            if (status == HC_SR_EDGE_OK) {
                S.n = type == 'p' ? 2 : nl.n;
                put(S, 0, nl, 0);
                if (nl.n == 2) put(S, 1, nl, 1);
                if (nl.len1 > 0) atomicMax(&W.ext[4 * c], (unsigned long long)nl.len1);  // :239-240
                if (nl.len2 > 0) atomicMax(&W.ext[4 * c + 1], (unsigned long long)nl.len2);
                if (type == 'p') {
                    status = lay_node(st, 'r', base_ID, base_len1, node_fwd, e, nl);
                    if (status == HC_SR_EDGE_OK) {
                        put(S, 1, nl, 0);
                        if (nl.len1 > 0) atomicMax(&W.ext[4 * c + 2], (unsigned long long)nl.len1);
                        if (nl.len2 > 0) atomicMax(&W.ext[4 * c + 3], (unsigned long long)nl.len2);
                    }
                }
            }
        }
        // a failing vertex keeps its place in the clique's span (empty entries at 0): the clique is refused as a whole
        if (status != HC_SR_EDGE_OK) atomicMin(&W.failkey[c], (unsigned long long)((j - W.off[c]) << 8 | status));
    }
    W.slot[j] = S;
    W.ecnt[j] = S.n;
}

// position + 2^31 as the sort's 32 key bits; a position of 2^31 (minus INT32_MIN) is beyond int and fails the geometry
__device__ inline uint32_t biased(int64_t pos, bool& beyond) {
    const int64_t x = pos + (1ll << 31);
    beyond = x > 0xffffffffll;
    return beyond ? 0xffffffffu : (uint32_t)x;
}

__global__ __launch_bounds__(256) void sr_clique_entry_kernel(SrCliqueView W) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= W.N) return;
    const uint32_t n = (uint32_t)W.ecnt[j];
    if (!n) return;
    const uint64_t c = W.key[j] >> 32;
    const uint64_t a = W.off[c], sz = W.off[c + 1] - a, r = j - a;
    const uint64_t ss = W.eoff[a], se = W.eoff[a + sz], pl0 = W.pl_first[c];
    const SrCliqueSlot& S = W.slot[j];
    const bool paired = W.type[c] == 'p';
    bool beyond = false;
    for (uint32_t m = 0; m < n; m++) {
        // 's': insertion number = the entry's rank among the clique's; 'p': one entry per vertex and layout
        // (the base is insertion 0 whatever its rank, :77-80; the vertices before it move up by its one entry)
        const uint64_t br = W.base_rank[c];
        const uint64_t ins = r == br ? 0 : (W.eoff[j] - ss) + m + (r < br ? 1 : 0);
        const uint64_t dest = paired ? ss + m * sz + (sz - 1 - r) : se - 1 - ins;
        bool bey;
        W.ekey_in[dest] = (pl0 + (paired ? m : 0)) << 32 | biased(S.pos[m], bey);
        W.eval_in[dest] = (uint32_t)(2 * j + m);
        beyond = beyond || bey;
    }
    if (beyond) atomicOr(&W.geom[c], 1u);
    if (r == W.base_rank[c]) {
        W.pl[pl0] = SrCliquePl{ss, (uint32_t)(paired ? sz : se - ss), (uint32_t)c, 0, S.len[0]};
        if (paired) W.pl[pl0 + 1] = SrCliquePl{ss + sz, (uint32_t)sz, (uint32_t)c, 1, S.len[1]};
    }
}

__global__ __launch_bounds__(256) void sr_clique_geometry_kernel(SrCliqueView W, uint64_t n_entries) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const uint64_t pl = W.ekey[i] >> 32;
    const SrCliquePl P = W.pl[pl];
    const uint64_t c = P.clique;
    const uint32_t slot = W.eval[i], f = W.eval[P.start], l = W.eval[P.start + P.n - 1];
    const SrCliqueSlot& S = W.slot[slot >> 1];
    const int64_t pos = S.pos[slot & 1], len = S.len[slot & 1];
    const int64_t minpos = W.slot[f >> 1].pos[f & 1], lastpos = W.slot[l >> 1].pos[l & 1];
    const int64_t total = (int64_t)P.base_len + (int64_t)W.ext[4 * c + 2 * P.which] + (int64_t)W.ext[4 * c + 2 * P.which + 1];  // :244
    bool bad = total > INT32_MAX || !(total > lastpos);                                                                      // :246
    const int64_t p = pos - (minpos < 0 ? minpos : 0);                                                                        // :248-252
    if (i == P.start) {
        bad = bad || len > total;  // :259
        W.pl_total[pl] = (int32_t)(total > INT32_MAX ? INT32_MAX : total);
    } else {
        bad = bad || p + len > total;  // :281 (p >= 0 and ascending by construction: :263-264)
    }
    if (bad) atomicOr(&W.geom[c], 1u);
    hc_sr_member m = S.m[slot & 1];
    m.pos = (int32_t)p;
    W.fmem[i] = m;
    W.fvert[i] = (uint32_t)W.key[slot >> 1];
    const int64_t end = p + len;
    const int32_t endpos = end < 0 ? 0 : end > INT32_MAX ? INT32_MAX : (int32_t)end;
    W.fend[i] = endpos;
    W.fused[i] = 1;
    W.slotpos[slot] = (uint32_t)i;
    W.ekey_in[i] = pl << 32 | (uint32_t)endpos;  // the second sort: (layout, endpos), :607-616
    W.eval_in[i] = (uint32_t)i;
}

// filter_subreads' selection (:597-622) for one layout by one wave; W.ekey2 / W.eval2: the layout's entries by endpos, list order
// among equals.  sel[2 item + which]: 0 = not selected, 1 = selected, 2 = counted for the group under the walk.
__global__ __launch_bounds__(256) void sr_clique_filter_kernel(SrCliqueView W, uint64_t n_pl, const uint64_t* __restrict__ ekey2,
                                                               const uint32_t* __restrict__ eval2) {
    const uint64_t pl = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (pl >= n_pl) return;  // (wave-uniform, as every branch below)
    const SrCliquePl P = W.pl[pl];
    const uint64_t c = P.clique;
    const uint64_t sz = W.off[c + 1] - W.off[c];
    if (!srclique::is_filtered(sz, W.m) || W.failkey[c] != kNoFail || W.geom[c]) {
        if (lane == 0) W.pl_filter[pl] = HC_SR_FILTER_NONE;
        return;
    }
    const uint32_t num = srclique::filter_num(W.m), n = P.n, which = P.which;
    const uint64_t start = P.start;
    uint32_t* sel = W.sel;
    // the leftmost num / 2 entries and the base, :604-605
    const uint32_t left = min(num / 2, n);
    uint32_t cnt = 0;
    for (uint32_t b = 0; b < left; b += 64) {
        const uint32_t k = b + lane;
        bool got = false;
        if (k < left) got = atomicExch(&sel[2 * (uint64_t)(W.eval[start + k] >> 1) + which], 1u) == 0;
        cnt += __popcll(__ballot(got));
    }
    {
        bool got = false;
        if (lane == 0) got = atomicExch(&sel[2 * (W.off[c] + W.base_rank[c]) + which], 1u) == 0;
        cnt += __popcll(__ballot(got));
    }
    uint32_t need = num > cnt ? num - cnt : 0;
    uint32_t i = n;
    srclique::GroupStep step = srclique::kTakeGroup;
    while (need > 0 && i > 0) {  // :618-622, group by group from the largest endpos down
        const uint32_t ep = (uint32_t)ekey2[start + i - 1];
        uint32_t gs = i;
        while (gs > 0) {
            const int64_t idx = (int64_t)gs - 1 - lane;
            const unsigned long long same = __ballot(idx >= 0 && (uint32_t)ekey2[start + idx] == ep);
            const uint32_t run = ~same == 0 ? 64u : (uint32_t)(__ffsll((long long)~same) - 1);
            gs -= run;
            if (run < 64) break;
        }
        uint32_t g = 0;
        for (uint32_t b = gs; b < i; b += 64) {
            const uint32_t k = b + lane;
            bool got = false;
            if (k < i) got = atomicCAS(&sel[2 * (uint64_t)(W.eval[eval2[start + k]] >> 1) + which], 0u, 2u) == 0;
            g += __popcll(__ballot(got));
        }
        step = srclique::group_step(g, need, n);
        for (uint32_t b = gs; b < i; b += 64) {  // taken: 2 -> 1; cut: 2 -> 0
            const uint32_t k = b + lane;
            if (k < i) atomicCAS(&sel[2 * (uint64_t)(W.eval[eval2[start + k]] >> 1) + which], 2u, step == srclique::kTakeGroup ? 1u : 0u);
        }
        if (step != srclique::kTakeGroup) {
            if (step == srclique::kCutStable && lane == 0)  // an insertion sort is stable: the group from the back of the list order
                for (uint32_t k = i; k-- > gs && need > 0;)
                    if (atomicCAS(&sel[2 * (uint64_t)(W.eval[eval2[start + k]] >> 1) + which], 0u, 1u) == 0) need--;
            break;
        }
        need -= g;
        i = gs;
    }
    const uint32_t cls = srclique::filter_class(step);
    if (cls != HC_SR_FILTER_HOST)  // :626-635
        for (uint32_t k = lane; k < n; k += 64) W.fused[start + k] = atomicOr(&sel[2 * (uint64_t)(W.eval[start + k] >> 1) + which], 0u) != 0;
    if (lane == 0) W.pl_filter[pl] = (uint8_t)cls;
}

__global__ __launch_bounds__(256) void sr_clique_status_kernel(SrCliqueView W) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > W.C) return;
    if (c == W.C) {
        W.lay_cnt[c] = 0;
        W.mem_cnt[c] = 0;
        return;
    }
    const unsigned long long fk = W.failkey[c];
    const uint32_t status = fk != kNoFail ? (uint32_t)(fk & 0xff) : W.geom[c] ? HC_SR_EDGE_BAD_GEOMETRY : HC_SR_EDGE_OK;
    W.status[c] = status;
    W.lay_cnt[c] = status == HC_SR_EDGE_OK ? W.lay0[c] : 0;
    W.mem_cnt[c] = status == HC_SR_EDGE_OK ? W.eoff[W.off[c + 1]] - W.eoff[W.off[c]] : 0;
}

__global__ __launch_bounds__(256) void sr_clique_compact_kernel(SrCliqueView W, uint64_t n_entries) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const uint64_t pl = W.ekey[i] >> 32;
    const SrCliquePl P = W.pl[pl];
    const uint64_t c = P.clique;
    if (W.status[c] != HC_SR_EDGE_OK) return;
    const uint64_t d = W.mem_off[c] + (i - W.eoff[W.off[c]]);
    W.out_members[d] = W.fmem[i];
    W.out_vertex[d] = W.fvert[i];
    W.out_used[d] = W.fused[i];
    W.uflag[d] = W.fused[i];
    if (i == P.start) {
        const uint64_t L = W.first[c] + P.which;
        hc_sr_layout lay;
        lay.first_member = d;
        lay.n_members = P.n;
        lay.total_len = W.pl_total[pl];
        W.out_layouts[L] = lay;
        W.out_filter[L] = W.pl_filter[pl];
    }
}

// the USED members of every layout, with the layout's full total_len (:725-741)
__global__ __launch_bounds__(256) void sr_clique_consensus_input_kernel(SrCliqueView W, uint64_t n_layouts, uint64_t n_members, hc_sr_layout* __restrict__ layouts,
                                                                        hc_sr_member* __restrict__ members) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_members && W.out_used[t]) members[W.uoff[t]] = W.out_members[t];
    if (t < n_layouts) {
        const hc_sr_layout F = W.out_layouts[t];
        hc_sr_layout lay;
        lay.first_member = W.uoff[F.first_member];
        lay.n_members = (uint32_t)(W.uoff[F.first_member + F.n_members] - lay.first_member);
        lay.total_len = F.total_len;
        layouts[t] = lay;
    }
}

__global__ __launch_bounds__(256) void sr_clique_subread_kernel(SrCliqueView W, const SrLayoutInfo* __restrict__ info) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= W.N) return;
    const uint64_t c = W.key[j] >> 32;
    hc_sr_subread_info s{-1, -1, -1, -1};
    if (W.status[c] == HC_SR_EDGE_OK) {
        const uint64_t l0 = W.first[c];
        const bool paired = W.type[c] == 'p';
        const int32_t trim_pos1 = info[l0].ret, trim_pos2 = paired ? info[l0 + 1].ret : -1;
        const uint32_t n = W.slot[j].n;
        uint32_t i0 = W.slotpos[2 * j], i1 = n == 2 ? W.slotpos[2 * j + 1] : kNone;
        if (paired) {
            sub_place(trim_pos1, W.fmem[i0].pos, s.index1, s.startpos1);                      // :559-572
            if (trim_pos2 >= 0) sub_place(trim_pos2, W.fmem[i1].pos, s.index2, s.startpos2);  // :575-593
        } else {
            if (i1 < i0) {  // the first entry in list order, :541-574
                const uint32_t t = i0;
                i0 = i1;
                i1 = t;
            }
            sub_place(trim_pos1, W.fmem[i0].pos, s.index1, s.startpos1);
            if (n == 2) sub_place(trim_pos1, W.fmem[i1].pos, s.index2, s.startpos2);  // :544-558
        }
    }
    W.sub[j] = s;
}

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t sr_clique_launch_keys(const SrCliqueView& W, const uint32_t* nodes, uint64_t* key_in, hipStream_t s) {
    if (W.N) hipLaunchKernelGGL(sr_clique_key_kernel, grid_for(W.N), dim3(256), 0, s, W, nodes, key_in);
    if (W.C) hipLaunchKernelGGL(sr_clique_init_kernel, grid_for(W.C), dim3(256), 0, s, W);
    return hipGetLastError();
}
hipError_t sr_clique_launch_precheck(const StoreView& st, const SrCliqueView& W, hipStream_t s) {
    if (W.N) hipLaunchKernelGGL(sr_clique_precheck_kernel, grid_for(W.N), dim3(256), 0, s, st, W);
    return hipGetLastError();
}
hipError_t sr_clique_launch_bases(const SrCliqueView& W, hipStream_t s) {
    hipLaunchKernelGGL(sr_clique_base_kernel, grid_for(W.C + 1), dim3(256), 0, s, W);
    return hipGetLastError();
}
hipError_t sr_clique_launch_hits(const SrCliqueView& W, uint64_t n_records, hipStream_t s) {
    if (n_records) hipLaunchKernelGGL(sr_clique_hit_kernel, grid_for(n_records), dim3(256), 0, s, W, n_records);
    return hipGetLastError();
}
hipError_t sr_clique_launch_nodes(const StoreView& st, const SrCliqueView& W, hipStream_t s) {
    hipLaunchKernelGGL(sr_clique_node_kernel, grid_for(W.N + 1), dim3(256), 0, s, st, W);
    return hipGetLastError();
}
hipError_t sr_clique_launch_entries(const SrCliqueView& W, hipStream_t s) {
    if (W.N) hipLaunchKernelGGL(sr_clique_entry_kernel, grid_for(W.N), dim3(256), 0, s, W);
    return hipGetLastError();
}
hipError_t sr_clique_launch_geometry(const SrCliqueView& W, uint64_t n_entries, hipStream_t s) {
    if (n_entries) hipLaunchKernelGGL(sr_clique_geometry_kernel, grid_for(n_entries), dim3(256), 0, s, W, n_entries);
    return hipGetLastError();
}
hipError_t sr_clique_launch_filter(const SrCliqueView& W, uint64_t n_pl, const uint64_t* ekey2, const uint32_t* eval2, hipStream_t s) {
    if (n_pl) hipLaunchKernelGGL(sr_clique_filter_kernel, dim3((unsigned)((n_pl + 3) / 4)), dim3(256), 0, s, W, n_pl, ekey2, eval2);
    return hipGetLastError();
}
hipError_t sr_clique_launch_status(const SrCliqueView& W, hipStream_t s) {
    hipLaunchKernelGGL(sr_clique_status_kernel, grid_for(W.C + 1), dim3(256), 0, s, W);
    return hipGetLastError();
}
hipError_t sr_clique_launch_compact(const SrCliqueView& W, uint64_t n_entries, hipStream_t s) {
    if (n_entries) hipLaunchKernelGGL(sr_clique_compact_kernel, grid_for(n_entries), dim3(256), 0, s, W, n_entries);
    return hipGetLastError();
}
hipError_t sr_clique_launch_consensus_input(const SrCliqueView& W, uint64_t n_layouts, uint64_t n_members, hc_sr_layout* layouts, hc_sr_member* members,
                                            hipStream_t s) {
    const uint64_t n = n_layouts > n_members ? n_layouts : n_members;
    if (n) hipLaunchKernelGGL(sr_clique_consensus_input_kernel, grid_for(n), dim3(256), 0, s, W, n_layouts, n_members, layouts, members);
    return hipGetLastError();
}
hipError_t sr_clique_launch_subreads(const SrCliqueView& W, const SrLayoutInfo* info, hipStream_t s) {
    if (W.N) hipLaunchKernelGGL(sr_clique_subread_kernel, grid_for(W.N), dim3(256), 0, s, W, info);
    return hipGetLastError();
}

}  // namespace hc
