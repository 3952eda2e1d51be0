// hc_br_kernels.hip — the device side of hc_br_evidence (include/hcsr.h): BranchReduction::findBranchingEvidence with buildDiffListOut,
// buildDiffListIn, findDiffPos and checkReadEvidence (reference src/BranchReduction.cpp:229-743) for every branch of the device graph.
// Integer and byte work in the count / exclusive-sum / expand idiom: a lane (or, for a pair of neighbour sequences, a wave) per item, its
// owner by bisection over an exclusive sum, never a global atomic.  The only racing stores write one value: a branch's
// HC_BR_BAD_ORIGINAL status and the two error flags.  Indices and arrays: hc_br.h; the width-dependent expressions: host/BranchEvidence.h.
//
// br_count_kernel      vertex and side -> is it a branch, its neighbours, its k (k - 1) / 2 pairs.
// br_in_keys_kernel    adj_in entry -> owner << 32 | source, for the sort that is sortAdjLists (:47).
// br_branches_kernel   after the three sums: branch b -> its vertex and where its neighbours and pairs begin.
// br_slots_kernel      neighbour -> its record (adj_out is in target order: the out-branch's own entry, or for an in-branch the first
//                      node -> node1 record by bisection), pos1, its read's sequence, length and pairedness.
// br_geometry_kernel   branch -> the paired-neighbour assert, max_pos and the start positions (:573-576), node1_len (:565-567).
// br_pairs_kernel      a WAVE per pair: the inclusion test, then the overlap 64 positions at a time (an in-branch from the back), the
//                      differing lanes ranked by ballot and prefix popcount, at most 100 positions in order, the i == 0 distance term.
// br_verdict_kernel    branch -> status (the first pair that fails), dist, the false mark, who leaves final_branch; the pairs' counts of a
//                      failed branch become 0; the neighbours' dict sizes.
// br_diff_*            after the sum and the sort of branch << 32 | (position + 2^31): first of every run, gather, offsets by bisection.
// br_items_kernel      item -> its neighbour and branch by bisection, id and mate id in the dict of node1 by binary search, the covered
//                      range of the diff list by binary search, the bases; up to two keys record << 33 | id << 1 | side.
// br_ev_*              after the sort: first of every run, the intersection where both sides stored the record, gather, offsets.
// br_missing_kernel    after the selection over the pairs: the missing-edge records (:476-511, :630-665).
// br_assemble_kernel   branch -> its hc_br_branch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_br.h"

namespace hc {
namespace br {
namespace {

constexpr uint32_t kBlock = 256;

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the largest j in [0, n) with a[j] <= x, for a[0] <= x < a[n - 1 + 1] and ascending a (n + 1 entries: n owners and the end)
__device__ inline uint64_t owner(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
__device__ inline uint64_t owner32(const uint32_t* __restrict__ a, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the first index in [0, n) whose value is not below x (n: none)
template <typename T, typename X>
__device__ inline uint64_t lower_bound(const T* __restrict__ a, uint64_t n, X x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// pair q of a branch of k neighbours -> (i, j), i < j, in (i, j) order
__device__ inline void pair_of(uint64_t q, uint32_t k, uint32_t* i_out, uint32_t* j_out) {
    uint32_t i = 0;
    while (q >= (uint64_t)(k - 1 - i)) q -= k - 1 - i, i++;
    *i_out = i;
    *j_out = i + 1 + (uint32_t)q;
}

__global__ __launch_bounds__(256) void br_count_kernel(In I, Work W) {
    const uint64_t t = gid(), V = I.g.V;
    if (t > 2 * V) return;
    uint64_t deg = 0;
    if (t < V) deg = I.g.in_off[t + 1] - I.g.in_off[t];
    else if (t < 2 * V) deg = I.g.out_off[t - V + 1] - I.g.out_off[t - V];
    const bool branch = deg > 1;
    W.cnt_b[t] = branch;
    W.cnt_s[t] = branch ? deg : 0;
    W.cnt_p[t] = branch ? deg * (deg - 1) / 2 : 0;
}

__global__ __launch_bounds__(256) void br_in_keys_kernel(In I, Work W) {
    const uint64_t i = gid();
    if (i >= I.g.E) return;
    W.in_key_a[i] = owner(I.g.in_off, I.g.V, i) << 32 | I.g.in_nodes[i];
}

__global__ __launch_bounds__(256) void br_branches_kernel(In I, Work W) {
    const uint64_t t = gid(), V = I.g.V;
    if (t > 2 * V) return;
    if (t == 2 * V) {
        W.nb_off[W.n_b] = W.cnt_s[t];
        W.pair_off[W.n_b] = W.cnt_p[t];
        return;
    }
    if (W.cnt_b[t + 1] == W.cnt_b[t]) return;
    const uint64_t b = W.cnt_b[t];
    W.br_node[b] = (uint32_t)(t < V ? t : t - V);
    W.nb_off[b] = W.cnt_s[t];
    W.pair_off[b] = W.cnt_p[t];
}

__global__ __launch_bounds__(256) void br_slots_kernel(In I, Work W) {
    const uint64_t s = gid();
    if (s >= W.n_s) return;
    const uint64_t b = owner(W.nb_off, W.n_b, s), i = s - W.nb_off[b];
    const uint32_t node1 = W.br_node[b];
    const bool outbranch = b >= W.n_in;
    uint32_t node2;
    uint64_t rec;
    bool ok = true;
    if (outbranch) {
        rec = I.g.out_off[node1] + i;
        node2 = (uint32_t)I.g.edges[rec].v2;
    } else {
        node2 = (uint32_t)W.in_key_b[I.g.in_off[node1] + i];
        // getEdgeInfo(node2, node1): the first record with that target; the list is in target order
        uint64_t lo = I.g.out_off[node2], hi = I.g.out_off[node2 + 1];
        const uint64_t end = hi;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (I.g.edges[mid].v2 < node1) lo = mid + 1;
            else hi = mid;
        }
        rec = lo;
        if (rec >= end || I.g.edges[rec].v2 != node1) ok = false, rec = 0;
    }
    uint32_t len = 0, olen = 0, paired = 0;
    uint64_t seq = 0;
    int32_t pos = 0;
    if (ok) {
        const hc_edge_rec e = I.g.edges[rec];
        pos = e.pos1;
        const uint32_t r = outbranch ? e.read2 : e.read1;
        if (r >= I.st.n_reads || (!outbranch && e.read2 >= I.st.n_reads)) {
            ok = false;
        } else {
            const uint32_t f = I.st.first[r];
            paired = I.st.first[r + 1] - f == 2;
            seq = I.st.off[f];
            len = (uint32_t)(I.st.off[f + 1] - seq);
            if (!outbranch) {  // edge->get_read(2)->get_len(), :566
                const uint32_t f2 = I.st.first[e.read2], n2 = I.st.first[e.read2 + 1] - f2;
                olen = (uint32_t)(I.st.off[f2 + n2] - I.st.off[f2]);
            }
        }
    }
    if (!ok) W.counters[kCntArgError] = 1;
    W.sl_node[s] = node2;
    W.sl_rec[s] = (uint32_t)rec;
    W.sl_pos[s] = pos;
    W.sl_seq[s] = seq;
    W.sl_len[s] = len;
    W.sl_olen[s] = olen;
    W.sl_paired[s] = (uint8_t)paired;
}

__global__ __launch_bounds__(256) void br_geometry_kernel(In I, Work W) {
    const uint64_t b = gid();
    if (b >= W.n_b) return;
    const uint64_t s0 = W.nb_off[b], s1 = W.nb_off[b + 1];
    const bool outbranch = b >= W.n_in;
    bool paired = false;
    int32_t max_pos = INT32_MIN;
    uint32_t node1_len = 0;
    for (uint64_t s = s0; s < s1; s++) {
        paired |= W.sl_paired[s] != 0;
        max_pos = max(max_pos, W.sl_pos[s]);
        if (node1_len == 0) node1_len = W.sl_olen[s];
    }
    for (uint64_t s = s0; s < s1; s++) W.sl_start[s] = outbranch ? W.sl_pos[s] : (int32_t)((uint32_t)max_pos - (uint32_t)W.sl_pos[s]);
    W.br_status[b] = paired ? HC_BR_PAIRED_NEIGHBOUR : HC_BR_OK;
    W.br_node1len[b] = node1_len;
}

// One wave per pair.  Everything but the byte comparison is wave-uniform.
__global__ __launch_bounds__(256) void br_pairs_kernel(In I, Work W) {
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= W.n_p) return;
    const uint64_t b = owner(W.pair_off, W.n_b, p);
    const uint64_t s0 = W.nb_off[b];
    const uint32_t k = (uint32_t)(W.nb_off[b + 1] - s0);
    uint32_t info = 0, cnt = 0;
    int32_t term = 0, rel = 0, len = 0;
    if (W.br_status[b] == HC_BR_OK) {
        uint32_t i, j;
        pair_of(p - W.pair_off[b], k, &i, &j);
        const uint64_t si = s0 + i, sj = s0 + j;
        const bool outbranch = b >= W.n_in, fwd = I.vfwd[W.br_node[b]] != 0;
        const int32_t pos_i = W.sl_start[si], pos_j = W.sl_start[sj];
        // a: the sequence that is entered at relative_pos, b: the one compared from its start
        const bool a_is_i = pos_i < pos_j;
        const uint64_t sa = a_is_i ? si : sj, sb = a_is_i ? sj : si;
        const uint64_t La = W.sl_len[sa], Lb = W.sl_len[sb];
        rel = a_is_i ? (int32_t)((uint32_t)pos_j - (uint32_t)pos_i) : (int32_t)((uint32_t)pos_i - (uint32_t)pos_j);
        const int32_t startpos = a_is_i ? pos_j : pos_i;
        if (W.sl_node[si] == W.sl_node[sj]) {
            info = HC_BR_REPEATED_NEIGHBOUR << kPairFailShift;  // :446
        } else if (rel > size_minus_min_overlap(La, I.min_overlap_len)) {
            info = outbranch ? kPairMissing | (a_is_i ? kPairMissingI : 0u) : HC_BR_BAD_GEOMETRY << kPairFailShift;  // :449-452, :605
        } else if (rel < 0 || (uint64_t)rel >= La || Lb == 0) {
            info = HC_BR_BAD_GEOMETRY << kPairFailShift;  // len == 0 (:471, :625), or substr throws
        } else {
            len = (int32_t)min(La - (uint64_t)rel, Lb);
            const uint8_t* A = I.st.bases + W.sl_seq[sa];
            const uint8_t* B = I.st.bases + W.sl_seq[sb];
            int32_t* slots = W.pr_diff + p * HC_BR_MAX_DIFFS;
            uint32_t first_t = 0;
            for (uint32_t base = 0; base < (uint32_t)len && cnt < HC_BR_MAX_DIFFS; base += 64) {
                const uint32_t t = base + lane;  // position in the compared (for an in-branch: reversed) substrings
                bool diff = false;
                if (t < (uint32_t)len) {
                    const uint32_t x = outbranch ? t : (uint32_t)len - 1 - t;
                    diff = oriented(A, La, fwd, (uint64_t)rel + x) != oriented(B, Lb, fwd, x);
                }
                const unsigned long long mask = __ballot(diff);
                if (mask == 0) continue;
                const uint32_t rank = cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
                if (diff && rank < HC_BR_MAX_DIFFS)
                    slots[rank] = outbranch ? (int32_t)(t + (uint32_t)startpos) : (int32_t)((uint32_t)len - t + (uint32_t)startpos);  // :473, :627
                if (cnt == 0) first_t = base + (uint32_t)__builtin_ctzll(mask);
                cnt = min(cnt + (uint32_t)__popcll(mask), HC_BR_MAX_DIFFS);
            }
            if (cnt == 0) {
                info = kPairIdentical;
            } else if (i == 0) {
                if (outbranch) {
                    term = (int32_t)(first_t + (uint32_t)startpos);  // :516
                } else {  // :600-602, :670
                    const uint64_t oi = W.sl_len[si] - (uint64_t)(int64_t)W.sl_pos[si], oj = W.sl_len[sj] - (uint64_t)(int64_t)W.sl_pos[sj];
                    term = (int32_t)(first_t + W.br_node1len[b] - (uint32_t)min(oi, oj));
                }
            }
        }
    }
    if (lane == 0) {
        W.pr_raw[p] = cnt;
        W.pr_info[p] = info;
        W.pr_term[p] = term;
        W.pr_rel[p] = rel;
        W.pr_len[p] = len;
    }
}

__global__ __launch_bounds__(256) void br_verdict_kernel(In I, Work W) {
    const uint64_t b = gid();
    if (b >= W.n_b) return;
    const uint64_t s0 = W.nb_off[b], p0 = W.pair_off[b], p1 = W.pair_off[b + 1];
    const uint32_t k = (uint32_t)(W.nb_off[b + 1] - s0);
    uint32_t status = W.br_status[b];  // HC_BR_PAIRED_NEIGHBOUR from the geometry pass, HC_BR_BAD_ORIGINAL from an earlier item pass
    bool is_false = false, any_missing = false, any_term = false;
    int32_t mn = 0, mx = 0;
    for (uint32_t n = 0; n < k; n++) W.sl_keep[s0 + n] = 1;
    if (status == HC_BR_OK) {
        uint32_t i = 0, j = 1;
        for (uint64_t p = p0; p < p1; p++) {
            const uint32_t info = W.pr_info[p];
            if (info >> kPairFailShift) {
                status = info >> kPairFailShift;
                break;
            }
            if (info & kPairIdentical) is_false = true;
            else if (info & kPairMissing) any_missing = true, W.sl_keep[s0 + (info & kPairMissingI ? i : j)] = 0;
            else if (i == 0) {
                const int32_t t = W.pr_term[p];
                mn = any_term ? min(mn, t) : t;
                mx = any_term ? max(mx, t) : t;
                any_term = true;
            }
            if (++j == k) i++, j = i + 1;
        }
    }
    const bool ok = status == HC_BR_OK, cleared = any_missing && k == 2;  // :330-332
    for (uint64_t p = p0; p < p1; p++) {
        W.pr_cnt[p] = ok ? W.pr_raw[p] : 0;
        W.pr_miss[p] = ok && (W.pr_info[p] & kPairIdentical);
    }
    const bool items = ok || status == HC_BR_BAD_ORIGINAL;  // the branch reached the evidence loop
    for (uint32_t n = 0; n < k; n++) {
        const uint64_t s = s0 + n;
        if (!ok || cleared) W.sl_keep[s] = 0;
        const uint32_t r = I.vread[W.sl_node[s]];
        W.sl_items[s] = items ? I.d.off[r + 1] - I.d.off[r] : 0;
    }
    W.br_status[b] = status;
    W.br_status8[b] = (uint8_t)status;
    W.br_false[b] = ok && is_false;
    W.br_dist[b] = ok && any_term ? half_toward_zero(mn, mx) : 0;
    if (b == 0) W.pr_cnt[W.n_p] = 0, W.sl_items[W.n_s] = 0;
}

__global__ __launch_bounds__(256) void br_diff_keys_kernel(Work W, uint64_t n_d) {
    const uint64_t d = gid();
    if (d >= n_d) return;
    const uint64_t p = owner32(W.pr_off, W.n_p, (uint32_t)d), b = owner(W.pair_off, W.n_b, p);
    const uint32_t v = (uint32_t)W.pr_diff[p * HC_BR_MAX_DIFFS + (d - W.pr_off[p])] + 0x80000000u;
    W.dk_in[d] = b << 32 | v;
}

__global__ __launch_bounds__(256) void br_diff_first_kernel(Work W, uint64_t n_d) {
    const uint64_t d = gid();
    if (d >= n_d) return;
    W.d_flag[d] = d == 0 || W.dk[d - 1] != W.dk[d];
}

__global__ __launch_bounds__(256) void br_diff_gather_kernel(Work W, uint64_t n_d) {
    const uint64_t u = gid();
    if (u >= n_d || u >= W.counters[kCntDiffSel]) return;
    const uint64_t key = W.dk[W.d_sel[u]];
    W.t_diff[u] = (int32_t)((uint32_t)key - 0x80000000u);
    W.d_branch[u] = (uint32_t)(key >> 32);
}

__global__ __launch_bounds__(256) void br_diff_offsets_kernel(Work W) {
    const uint64_t b = gid();
    if (b > W.n_b) return;
    W.diff_off[b] = lower_bound(W.d_branch, W.counters[kCntDiffSel], (uint32_t)b);
}

__global__ __launch_bounds__(256) void br_nb_gather_kernel(Work W) {
    const uint64_t u = gid();
    if (u >= W.n_s || u >= W.counters[kCntNbSel]) return;
    W.t_nb[u] = W.sl_node[W.nb_sel[u]];
}

__global__ __launch_bounds__(256) void br_items_kernel(In I, Work W, uint64_t n_items) {
    const uint64_t t = gid();
    if (t >= n_items) return;
    const uint64_t invalid = (uint64_t)I.g.E << 33 | 0x1ffffffffull;  // behind every record's keys after the sort
    uint64_t key1 = invalid, key2 = invalid;
    const uint64_t s = owner(W.sl_item_off, W.n_s, t), b = owner(W.nb_off, W.n_b, s);
    if (W.br_status[b] == HC_BR_OK) {
        const uint32_t node1 = W.br_node[b], node2 = W.sl_node[s];
        const hc_sr_original e = I.d.entries[I.d.off[I.vread[node2]] + (t - W.sl_item_off[s])];
        const uint64_t d1 = I.d.off[I.vread[node1]], n1 = I.d.off[I.vread[node1] + 1] - d1;
        const hc_sr_original* s1 = I.d.entries + d1;
        auto in_subreads1 = [&](uint64_t id) {
            uint64_t lo = 0, hi = n1;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (s1[mid].id < id) lo = mid + 1;
                else hi = mid;
            }
            return lo < n1 && s1[lo].id == id;
        };
        const uint64_t id = e.id;
        uint64_t mate = 0;
        const bool common = in_subreads1(id), common_pe = mate_of(id, I.se, I.pe, &mate) && in_subreads1(mate);
        if (common || common_pe) {
            bool bad = id >= I.o.n;  // get_read, :288 / :306
            if (!bad) {
                const uint64_t oa = I.o.off[id], olen = I.o.off[id + 1] - oa, L = W.sl_len[s];
                const uint8_t* ob = I.o.bases + oa;
                const uint8_t* cb = I.st.bases + W.sl_seq[s];
                const bool fwd1 = I.vfwd[node1] != 0;
                const int32_t startpos = W.sl_start[s];
                const int32_t read_start = (int32_t)((uint32_t)startpos + (uint32_t)e.index1), read_end = int_plus_size(read_start, olen);
                const int32_t contig_end = int_plus_size(startpos, L);
                const int32_t lo = max(read_start, startpos), hi = min(read_end, contig_end);
                const int32_t* dl = W.t_diff + W.diff_off[b];
                const uint64_t nd = W.diff_off[b + 1] - W.diff_off[b];
                bool result = false;
                if (lo < hi) {
                    uint64_t u = lower_bound(dl, nd, lo);
                    const uint64_t u_end = lower_bound(dl, nd, hi);
                    result = u < u_end;
                    for (; u < u_end; u++) {
                        const uint64_t xr = (uint32_t)(dl[u] - read_start), xc = (uint32_t)(dl[u] - startpos);
                        if (xr >= olen || xc >= L || oriented(ob, olen, e.forward != 0, xr) != oriented(cb, L, fwd1, xc)) {
                            result = false;
                            break;
                        }
                    }
                }
                if (result) {
                    const uint64_t rec = W.sl_rec[s], side = b >= W.n_in;
                    if (common) {
                        if (id < 2 * I.orc) key1 = rec << 33 | id << 1 | side;
                        else bad = true;  // :300
                    }
                    if (common_pe) {
                        const uint64_t joint = I.orc + min(id, mate);
                        if (joint < 2 * I.orc) key2 = rec << 33 | joint << 1 | side;
                        else bad = true;  // :319
                    }
                }
            }
            if (bad) {
                key1 = key2 = invalid;
                W.br_status[b] = HC_BR_BAD_ORIGINAL;  // (every writer writes this value; the call runs B - D again with it)
                W.counters[kCntBadOriginal] = 1;
            }
        }
    }
    W.ek_in[2 * t] = key1;
    W.ek_in[2 * t + 1] = key2;
}

__global__ __launch_bounds__(256) void br_record_flags_kernel(Work W) {
    const uint64_t s = gid();
    if (s >= W.n_s || !W.sl_keep[s]) return;
    const uint64_t b = owner(W.nb_off, W.n_b, s);
    const uint32_t rec = W.sl_rec[s];
    (b >= W.n_in ? W.rec_out : W.rec_in)[rec] = 1;
    W.rec_flag[rec] = 1;  // (an in-slot and an out-slot of one record write the same value)
}

__global__ __launch_bounds__(256) void br_ev_keep_kernel(In I, Work W, uint64_t n_keys) {
    const uint64_t t = gid();
    if (t >= n_keys) return;
    const uint64_t key = W.ek[t], rec = key >> 33;
    bool keep = false;
    if (rec < I.g.E && (t == 0 || W.ek[t - 1] != key)) {
        const bool in = W.rec_in[rec], out = W.rec_out[rec], side = key & 1;
        if (in && out) {  // :367-384: an id of the in-branch's list that the out-branch's list has too
            if (!side) {
                const uint64_t u = lower_bound(W.ek, n_keys, key | 1);
                keep = u < n_keys && W.ek[u] == (key | 1);
            }
        } else {
            keep = side ? out : in;
        }
    }
    W.e_flag[t] = keep;
}

__global__ __launch_bounds__(256) void br_ev_gather_kernel(Work W, uint64_t n_keys) {
    const uint64_t u = gid();
    if (u >= n_keys || u >= W.counters[kCntEvSel]) return;
    const uint64_t key = W.ek[W.e_sel[u]];
    W.t_ev_ids[u] = (uint32_t)(key >> 1);
    W.e_rec[u] = (uint32_t)(key >> 33);
}

__global__ __launch_bounds__(256) void br_ev_edges_kernel(In I, Work W) {
    const uint64_t k = gid(), n = W.counters[kCntRecSel], n_ids = W.counters[kCntEvSel];
    if (k > n || k > I.g.E) return;
    if (k == n) {
        W.t_ev_off[k] = n_ids;
        return;
    }
    const uint32_t rec = W.rec_sel[k];
    W.t_ev_edge[2 * k] = (uint32_t)I.g.edges[rec].v1;
    W.t_ev_edge[2 * k + 1] = (uint32_t)I.g.edges[rec].v2;
    W.t_ev_off[k] = lower_bound(W.e_rec, n_ids, rec);
}

__global__ __launch_bounds__(256) void br_missing_kernel(In I, Work W) {
    const uint64_t u = gid();
    if (u >= W.n_p || u >= W.counters[kCntMissSel]) return;
    const uint64_t p = W.miss_sel[u], b = owner(W.pair_off, W.n_b, p), s0 = W.nb_off[b];
    uint32_t i, j;
    pair_of(p - W.pair_off[b], (uint32_t)(W.nb_off[b + 1] - s0), &i, &j);
    const bool outbranch = b >= W.n_in;
    // :489, :643: node_i first where pos_i < pos_j, or pos_i == pos_j and node_i < node_j (neighbours ascend and differ)
    const bool i_first = W.sl_start[s0 + i] <= W.sl_start[s0 + j];
    const uint64_t sa = s0 + (i_first ? i : j), sb = s0 + (i_first ? j : i);
    const hc_edge_rec ea = I.g.edges[W.sl_rec[sa]], eb = I.g.edges[W.sl_rec[sb]];
    uint64_t* raw = (uint64_t*)&W.t_missing[u];  // (the padding between read2 and v1 is part of the record's 80 bytes)
    for (int w = 0; w < 10; w++) raw[w] = 0;
    hc_edge_rec& e = W.t_missing[u];
    e.score = I.edge_threshold;
    e.mismatch_rate = -1;
    e.pos1 = W.pr_rel[p];
    e.ori1 = outbranch ? ea.ori2 : ea.ori1;
    e.ori2 = outbranch ? eb.ori2 : eb.ori1;
    e.ord = '-';
    e.read1 = outbranch ? ea.read2 : ea.read1;
    e.read2 = outbranch ? eb.read2 : eb.read1;
    e.v1 = W.sl_node[sa];
    e.v2 = W.sl_node[sb];
    e.perc = overlap_perc(W.pr_len[p], min(W.sl_len[sa], W.sl_len[sb]));
    e.len0 = e.len1 = W.pr_len[p];
}

__global__ __launch_bounds__(256) void br_assemble_kernel(Work W) {
    const uint64_t b = gid();
    if (b >= W.n_b) return;
    const uint64_t n_sel = W.counters[kCntNbSel];
    const uint64_t nb0 = lower_bound(W.nb_sel, n_sel, W.nb_off[b]), nb1 = lower_bound(W.nb_sel, n_sel, W.nb_off[b + 1]);
    hc_br_branch r;
    r.node = W.br_node[b];
    r.side = b >= W.n_in ? HC_BR_OUT : HC_BR_IN;
    r.status = (uint8_t)W.br_status[b];
    r.is_false = W.br_false[b];
    r.pad = 0;
    r.dist = W.br_dist[b];
    r.nb_count = (uint32_t)(nb1 - nb0);
    r.nb_first = nb0;
    r.diff_first = W.diff_off[b];
    r.diff_count = (uint32_t)(W.diff_off[b + 1] - W.diff_off[b]);
    r.n_neighbours = (uint32_t)(W.nb_off[b + 1] - W.nb_off[b]);
    W.t_branches[b] = r;
}

inline dim3 lanes(uint64_t n) { return dim3((uint32_t)((n + kBlock - 1) / kBlock ? (n + kBlock - 1) / kBlock : 1)); }  // (n < 2^32)

}  // namespace

#define HC_BR_LAUNCH(kernel, n, ...)                                                   \
    do {                                                                               \
        hipLaunchKernelGGL(kernel, lanes(n), dim3(kBlock), 0, s, __VA_ARGS__);         \
        return hipGetLastError();                                                      \
    } while (0)

hipError_t launch_count(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_count_kernel, 2 * (uint64_t)I.g.V + 1, I, W); }
hipError_t launch_in_keys(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_in_keys_kernel, I.g.E, I, W); }
hipError_t launch_branches(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_branches_kernel, 2 * (uint64_t)I.g.V + 1, I, W); }
hipError_t launch_slots(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_slots_kernel, W.n_s, I, W); }
hipError_t launch_branch_geometry(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_geometry_kernel, W.n_b, I, W); }
hipError_t launch_pairs(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_pairs_kernel, W.n_p * 64, I, W); }
hipError_t launch_branch_verdict(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_verdict_kernel, W.n_b, I, W); }
hipError_t launch_diff_keys(const Work& W, uint64_t n_d, hipStream_t s) { HC_BR_LAUNCH(br_diff_keys_kernel, n_d, W, n_d); }
hipError_t launch_diff_first(const Work& W, uint64_t n_d, hipStream_t s) { HC_BR_LAUNCH(br_diff_first_kernel, n_d, W, n_d); }
hipError_t launch_diff_gather(const Work& W, uint64_t n_d, hipStream_t s) { HC_BR_LAUNCH(br_diff_gather_kernel, n_d, W, n_d); }
hipError_t launch_diff_offsets(const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_diff_offsets_kernel, W.n_b + 1, W); }
hipError_t launch_nb_gather(const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_nb_gather_kernel, W.n_s, W); }
hipError_t launch_items(const In& I, const Work& W, uint64_t n_items, hipStream_t s) { HC_BR_LAUNCH(br_items_kernel, n_items, I, W, n_items); }
hipError_t launch_record_flags(const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_record_flags_kernel, W.n_s, W); }
hipError_t launch_ev_keep(const In& I, const Work& W, uint64_t n_keys, hipStream_t s) { HC_BR_LAUNCH(br_ev_keep_kernel, n_keys, I, W, n_keys); }
hipError_t launch_ev_gather(const Work& W, uint64_t n_keys, hipStream_t s) { HC_BR_LAUNCH(br_ev_gather_kernel, n_keys, W, n_keys); }
hipError_t launch_ev_edges(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_ev_edges_kernel, (uint64_t)I.g.E + 1, I, W); }
hipError_t launch_missing(const In& I, const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_missing_kernel, W.n_p, I, W); }
hipError_t launch_assemble(const Work& W, hipStream_t s) { HC_BR_LAUNCH(br_assemble_kernel, W.n_b, W); }

}  // namespace br
}  // namespace hc
