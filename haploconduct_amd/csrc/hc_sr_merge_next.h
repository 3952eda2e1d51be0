// hc_sr_merge_next.h — what the device kernels (hc_sr_merge_next_kernels.hip), the glue (hc_api_sr_merge_next.cpp) and the host mirror
// (host/SrMergeNext.cpp) of hc_sr_merge_next (include/hcsr.h) share: which super-read a pair owns, the member-to-vertex choice, the
// vertex tests in the reference's order, the index shift and the clique ordering after a self-merge, and the launch interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcsr.h"
#include "hc_sr_next.h"

namespace hc {
namespace mn {

constexpr uint8_t kNoEntry = 255;  // a kind sr_next_resolve refuses without reading anything: a pair without a super-read, a visited vertex
constexpr uint32_t kHeld = 16;     // status of a vertex that passed hc_sr_next's tests and went to the tips list: not kept (no HC_SR_NEXT_*)

// the call's inputs as one block of pointers (device pointers in the kernels, the caller's in the mirror)
struct In {
    const uint32_t* pairs;
    const uint32_t* pair_status;
    const uint64_t* first_layout;
    const hc_sr_layout* layouts;
    const hc_sr_member* members;
    const uint32_t* status;
    const uint64_t* out_off;
    const hc_sr_subread_info* subreads;
    const uint32_t* vertex_read;
    const uint8_t* vertex_fwd;
    const uint8_t* inclusions;  // may be null
    const uint8_t* tip_reads;   // may be null
    uint64_t n_pairs, n_layouts, n_members, n_vertices;
    uint32_t n_reads;
};

// The super-read of pair i as process_cliques sees it (src/SRBuilder.cpp:981-1001), before the self-overlap test: e.kind = SINGLE or
// PAIRED with the mates at out_off of its layouts (a layout that is not HC_SR_OK is an empty mate), or kNoEntry.  n_clique = members of
// the first layout (1..4).
__host__ __device__ inline void pair_entry(const In& I, uint64_t i, hc_sr_next_entry& e, uint32_t& n_clique) {
    e = hc_sr_next_entry{0, 0, 0, 0, 0, kNoEntry, HC_SR_SRC_CONSENSUS, HC_SR_SRC_CONSENSUS, 0};
    n_clique = 0;
    if (I.pair_status[i] != HC_SR_EDGE_OK) return;
    const uint32_t v = I.pairs[2 * i], w = I.pairs[2 * i + 1];
    if (v >= I.n_vertices || w >= I.n_vertices || v == w) return;
    const uint64_t l0 = I.first_layout[i], l1 = I.first_layout[i + 1];
    if (l1 < l0 || l1 > I.n_layouts || (l1 - l0 != 1 && l1 - l0 != 2)) return;
    const hc_sr_layout L = I.layouts[l0];
    if (L.n_members < 1 || L.n_members > 4 || L.first_member > I.n_members || L.n_members > I.n_members - L.first_member) return;
    uint64_t off[2] = {0, 0};
    uint32_t len[2] = {0, 0};
    for (uint64_t l = l0; l < l1; l++) {
        const uint64_t a = I.out_off[l], b = I.out_off[l + 1];
        if (b < a || b - a >= kNextMaxLen) return;
        off[l - l0] = a;
        len[l - l0] = I.status[l] == HC_SR_OK ? (uint32_t)(b - a) : 0u;
    }
    e.off1 = off[0];
    e.len1 = len[0];
    e.off2 = off[1];
    e.len2 = len[1];
    e.kind = l1 - l0 == 2 ? HC_SR_NEXT_PAIRED : HC_SR_NEXT_SINGLE;
    n_clique = L.n_members;
}

// the pair goes through merge_self_overlap (:983-985)
__host__ __device__ inline bool self_candidate(const hc_sr_next_entry& e) { return e.kind == HC_SR_NEXT_PAIRED && e.len1 && e.len2; }

// the vertex a member of pair (lo, hi)'s layout stands for
__host__ __device__ inline uint32_t member_vertex(const In& I, uint32_t lo, uint32_t hi, const hc_sr_member& m) {
    return I.vertex_read[lo] == m.read ? lo : hi;
}

// HC_SR_MN_* of a pair from its entry's status; self: merge_self_overlap merged it
__host__ __device__ inline uint32_t pair_kind(uint8_t entry_kind, uint32_t status, bool self) {
    if (entry_kind == kNoEntry || status == HC_SR_NEXT_BAD_ENTRY) return HC_SR_MN_NONE;
    if (status == HC_SR_NEXT_DROPPED_EMPTY) return HC_SR_MN_DROPPED_EMPTY;
    if (status != HC_SR_NEXT_KEPT) return HC_SR_MN_DROPPED_N_RATE;
    return self ? HC_SR_MN_SINGLE_SELF : entry_kind == HC_SR_NEXT_PAIRED ? HC_SR_MN_PAIRED : HC_SR_MN_SINGLE;
}

// HC_SR_MN_V_* of a vertex (:1283-1311): `status` = hc_sr_next's verdict on its trivial entry (short before N rate, hc_sr_next.h)
__host__ __device__ inline uint32_t vertex_state(bool visited, uint32_t status, bool ignore_inclusions, bool inclusion, bool store_tips, bool tip) {
    if (visited) return HC_SR_MN_V_MERGED;
    if (status == HC_SR_NEXT_DROPPED_SHORT) return HC_SR_MN_V_SHORT;    // :1286
    if (status == HC_SR_NEXT_DROPPED_N_RATE) return HC_SR_MN_V_N_RATE;  // :1292
    if (status != HC_SR_NEXT_KEPT) return HC_SR_MN_V_BAD;
    if (ignore_inclusions && inclusion) return HC_SR_MN_V_INCLUSION;  // :1298
    if (tip && store_tips) return HC_SR_MN_V_TIP;                     // :1305
    return HC_SR_MN_V_TRIVIAL;
}

// :918-922: new_index2 = index2 + seq1.length() - (seq1.length() - overlap_pos)
__host__ __device__ inline int32_t shift_index2(int32_t index2, int32_t overlap_pos) {
    return index2 >= 0 ? (int32_t)((uint32_t)index2 + (uint32_t)overlap_pos) : index2;
}

// new_sorted_clique (:913-935) of a self-merged pair: `first` = the vertex of the first layout's first member with its (shifted) info,
// `second` = the pair's other vertex.  The unordered_map iterates two keys in the reverse of their insertion order (:571), each key
// gives (key, index1) and, where index2 >= 0, (key, index2); the insertion sort keeps that order among equal indexes.  Returns the count.
__host__ __device__ inline uint32_t merged_clique(uint32_t first, const hc_sr_subread_info& fi, uint32_t second, const hc_sr_subread_info& si,
                                                  uint64_t out[4]) {
    uint32_t node[4];
    int32_t idx[4];
    uint32_t n = 0;
    node[n] = second, idx[n++] = si.index1;
    if (si.index2 >= 0) node[n] = second, idx[n++] = si.index2;
    node[n] = first, idx[n++] = fi.index1;
    if (fi.index2 >= 0) node[n] = first, idx[n++] = fi.index2;
    for (uint32_t a = 1; a < n; a++)
        for (uint32_t b = a; b > 0 && idx[b] < idx[b - 1]; b--) {
            const int32_t t = idx[b];
            idx[b] = idx[b - 1], idx[b - 1] = t;
            const uint32_t u = node[b];
            node[b] = node[b - 1], node[b - 1] = u;
        }
    for (uint32_t a = 0; a < n; a++) out[a] = node[a];
    return n;
}

// how many entries merged_clique lists for a pair's two infos as calcSubreadInfo left them (before the shift)
__host__ __device__ inline uint32_t merged_clique_size(const hc_sr_subread_info& a, const hc_sr_subread_info& b, int32_t overlap_pos) {
    return 2u + (shift_index2(a.index2, overlap_pos) >= 0) + (shift_index2(b.index2, overlap_pos) >= 0);
}

// clique (returns the count, at most 4) and the two subread entries of pair i's super-read; overlap_pos >= 0: it self-merged
__host__ __device__ inline uint32_t sr_tables(const In& I, uint64_t i, int32_t overlap_pos, uint64_t clique[4], hc_fno_subread sub[2]) {
    const uint32_t v = I.pairs[2 * i], w = I.pairs[2 * i + 1], lo = v < w ? v : w, hi = v < w ? w : v;
    hc_sr_subread_info s[2] = {I.subreads[2 * i], I.subreads[2 * i + 1]};
    if (overlap_pos >= 0)
        for (int k = 0; k < 2; k++) s[k].index2 = shift_index2(s[k].index2, overlap_pos);
    sub[0] = hc_fno_subread{lo, s[0].index1, s[0].index2, s[0].startpos1, s[0].startpos2};
    sub[1] = hc_fno_subread{hi, s[1].index1, s[1].index2, s[1].startpos1, s[1].startpos2};
    const hc_sr_layout L = I.layouts[I.first_layout[i]];
    if (overlap_pos >= 0) {
        const bool first_lo = member_vertex(I, lo, hi, I.members[L.first_member]) == lo;
        return first_lo ? merged_clique(lo, s[0], hi, s[1], clique) : merged_clique(hi, s[1], lo, s[0], clique);
    }
    for (uint32_t k = 0; k < L.n_members; k++) clique[k] = member_vertex(I, lo, hi, I.members[L.first_member + k]);
    return L.n_members;
}

// a merged pair's entry rewritten: (pair, its overlap_pos, where the kept form appended the merged read)
struct Rewrite {
    uint64_t off;
    uint32_t pair, len;
    int32_t overlap_pos;
    uint32_t pad;
};

// the slots of one call on the device: [0, n_pairs) the pairs, [n_pairs, n_pairs + n_vertices) the vertices
struct Slots {
    hc_sr_next_entry* entries;
    uint32_t* status;
    uint64_t *cnt, *bytes;  // hc_sr_next's: kept ? 1 | n_mates << 32 : 0, kept ? bytes : 0 (n_slots + 1)
    uint64_t* key;          // per slot what the rank sum adds up: pairs: single | paired << 32; vertices: trivial | tip << 32 (n_slots + 1)
    uint64_t* rank;         // its exclusive sum
    int32_t* overlap_pos;   // per pair, -1 unless self-merged
    uint8_t* n_clique;      // per pair
    uint8_t* visited;       // per vertex
};
struct Totals {  // read from rank[] by the host between the launches
    uint32_t n_singles, n_paired, n_trivials, n_tips;
};
// the tables in device memory, as hc_sr_merge_next_output names them
struct Tables {
    uint32_t* pair_kind;
    int32_t* pair_new_id;
    uint32_t* vertex_state;
    hc_fno_read* nodes;
    hc_fno_read* srs;
    uint32_t* sr_pair;
    uint64_t *clique_cnt, *clique_off, *clique_nodes, *subread_off;
    hc_fno_subread* subreads;
    uint32_t* tips;
};

// hc_sr_merge_next_kernels.hip; every launch is one kernel whatever the sizes
hipError_t launch_pairs(In I, Slots S, hipStream_t stream);
hipError_t launch_rewrite(const Rewrite* rw, uint64_t n, uint64_t n_pairs, Slots S, hipStream_t stream);
hipError_t launch_mark(In I, Slots S, hipStream_t stream);
hipError_t launch_vertices(In I, Slots S, SrNextSources src, hipStream_t stream);
hipError_t launch_vertex_finish(In I, Slots S, uint32_t ignore_inclusions, uint32_t store_tips, Tables T, hipStream_t stream);
// the surviving entries in final order into out_* (what hc_sr_set_next_reads' gather takes), ids, kinds, nodes, tips, sr_pair, clique counts
hipError_t launch_order(In I, Slots S, Totals N, SrNextSources src, hc_sr_next_entry* out_entries, uint32_t* out_status, uint64_t* out_cnt,
                        uint64_t* out_bytes, Tables T, hipStream_t stream);
hipError_t launch_tables(In I, Slots S, uint64_t n_srs, Tables T, hipStream_t stream);

}  // namespace mn

// hc_api_sr_next.cpp: the tail of hc_sr_set_next_reads from "the entries, their statuses and the two sums are on the device" on — the
// gather, the histograms, plan_store and finish_store —, shared with hc_sr_merge_next.  srn.entries / status / cnt_off / byte_off hold n
// entries; cn carries the counts so far and receives ms_plan and the second half of ms_device.
int sr_next_store(hc_ctx* c, uint64_t n, uint64_t n_extra, uint32_t n_kept, uint32_t n_seq, uint64_t total, hc_sr_next_counts& cn);
// hc_api_sr.cpp: hc_sr_merge_self_overlaps_kept behind its own checks
int sr_self_kept_run(hc_ctx* c, const char* me, const hc_sr_pair* pairs, uint64_t n_pairs, const hc_sr_self_settings* settings, int32_t* overlap_pos,
                     double* score, uint32_t* status, uint64_t* out_off, uint64_t* n_out, hc_sr_self_stats* stats);

}  // namespace hc
