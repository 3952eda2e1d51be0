// hc_sr_clique_next.h — what the device kernels (hc_sr_clique_next_kernels.hip), the glue (hc_api_sr_clique_next.cpp) and the host mirror
// (host/SrCliqueNext.cpp) of hc_sr_clique_next (include/hcsr.h) share: which super-read a clique owns, who owns a member, where a vertex's
// subread info lies, the pre-order of a self-merged clique's index entries, and the launch interface.  The rules a clique shares with a
// pair — pair_kind, vertex_state, shift_index2, the slots and the vertex kernels — are those of hc_sr_merge_next.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/hcsr.h"
#include "hc_sr_merge_next.h"

namespace hc {
namespace cn {

constexpr uint32_t kNone = 0xffffffffu;

// the call's inputs as one block of pointers (device pointers in the kernels, the caller's in the mirror)
struct In {
    const uint64_t* clique_off;
    const uint32_t* clique_nodes;
    const uint32_t* clique_status;
    const uint64_t* first_layout;
    const hc_sr_layout* layouts;
    const uint32_t* member_vertex;
    const uint32_t* status;
    const uint64_t* out_off;
    const hc_sr_subread_info* subreads;
    uint64_t n_cliques, n_items, n_layouts, n_members, n_vertices;
};

// The super-read of clique i as process_cliques sees it (src/SRBuilder.cpp:981-1001), before the self-overlap test, from the clique's own
// few numbers (no walk over its vertices: the vertex range test is `bad`, decided by the host's one pass, vertices_ok below):
// e.kind = SINGLE or PAIRED with the mates at out_off of its layouts (a layout that is not HC_SR_OK is an empty mate), or mn::kNoEntry.
__host__ __device__ inline void clique_entry(const In& I, uint64_t i, bool bad, hc_sr_next_entry& e) {
    e = hc_sr_next_entry{0, 0, 0, 0, 0, mn::kNoEntry, HC_SR_SRC_CONSENSUS, HC_SR_SRC_CONSENSUS, 0};
    if (bad || I.clique_status[i] != HC_SR_EDGE_OK) return;
    if (I.clique_off[i + 1] - I.clique_off[i] < 2) return;  // (clique_off ascends: checked for the whole call)
    const uint64_t l0 = I.first_layout[i], l1 = I.first_layout[i + 1];
    if (l1 < l0 || l1 > I.n_layouts || (l1 - l0 != 1 && l1 - l0 != 2)) return;
    uint64_t off[2] = {0, 0};
    uint32_t len[2] = {0, 0};
    for (uint64_t l = l0; l < l1; l++) {
        const hc_sr_layout L = I.layouts[l];
        if (L.first_member > I.n_members || L.n_members > I.n_members - L.first_member) return;
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
}

// The host's pass over a clique that clique_entry accepts: every clique vertex and every vertex of the first layout's members lies
// inside the graph (visited[] and find-next-overlaps index by them).
inline bool vertices_ok(const In& I, uint64_t i) {
    for (uint64_t j = I.clique_off[i]; j < I.clique_off[i + 1]; j++)
        if (I.clique_nodes[j] >= I.n_vertices) return false;
    const hc_sr_layout L = I.layouts[I.first_layout[i]];
    for (uint64_t m = L.first_member; m < L.first_member + L.n_members; m++)
        if (I.member_vertex[m] >= I.n_vertices) return false;
    return true;
}

// The first layouts of the cliques that own an entry, in clique order: where the member range starts, how long it is, whose it is.  The
// host lists them (the ranges must ascend without overlap: HC_ERR_ARG otherwise), a member's lane bisects them for its owner.
struct Owner {
    uint64_t first_member;
    uint32_t n_members, clique;
};
// the owner of member m among n ascending ranges, or kNone
__host__ __device__ inline uint32_t owner_of(const Owner* own, uint64_t n, uint64_t m) {
    uint64_t lo = 0, hi = n;  // the last range that starts at or before m
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (own[mid].first_member <= m) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return kNone;
    const Owner o = own[lo - 1];
    return m - o.first_member < o.n_members ? (uint32_t)(lo - 1) : kNone;
}

// The host's one pass over the cliques, shared by the glue and the mirror: bad[i] and the owners' list.  false: the owners' member
// ranges do not ascend.
inline bool host_plan(const In& I, std::vector<uint8_t>& bad, std::vector<Owner>& own) {
    bad.assign(I.n_cliques ? I.n_cliques : 1, 0);
    own.clear();
    uint64_t end = 0;
    for (uint64_t i = 0; i < I.n_cliques; i++) {
        hc_sr_next_entry e;
        clique_entry(I, i, false, e);
        if (e.kind == mn::kNoEntry) continue;
        if (!vertices_ok(I, i)) {
            bad[i] = 1;
            continue;
        }
        const hc_sr_layout L = I.layouts[I.first_layout[i]];
        if (L.first_member < end) return false;
        end = L.first_member + L.n_members;
        own.push_back(Owner{L.first_member, L.n_members, (uint32_t)i});
    }
    return true;
}

// the clique of item j of clique_nodes: the last i with clique_off[i] <= j (empty cliques own nothing)
__host__ __device__ inline uint64_t clique_of_item(const uint64_t* clique_off, uint64_t n_cliques, uint64_t j) {
    uint64_t lo = 0, hi = n_cliques;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (clique_off[mid + 1] <= j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__host__ __device__ inline uint64_t item_key(uint64_t clique, uint32_t vertex) { return clique << 32 | vertex; }

// where vertex x of clique i lies among the sorted keys [a, b) of the clique — and so its entry of `subreads` — or kNone
__host__ __device__ inline uint32_t find_vertex(const uint64_t* key, uint64_t a, uint64_t b, uint64_t clique, uint32_t x) {
    const uint64_t want = item_key(clique, x);
    uint64_t lo = a, hi = b;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < b && key[lo] == want ? (uint32_t)lo : kNone;
}

// index entries a member's vertex gives new_sorted_clique (:917, :918-922): its info's index1 and, where index2 >= 0, index2
__host__ __device__ inline uint32_t member_items(const hc_sr_subread_info& s) { return 1u + (s.index2 >= 0); }

// the sort key of an index entry of super-read k: ascending index inside the super-read
__host__ __device__ inline uint64_t index_key(uint64_t k, int32_t index) { return k << 32 | (uint32_t)((uint32_t)index + 0x80000000u); }

// the blocks of one call on the device besides mn::Slots ([0, n_cliques) the cliques, then the vertices)
struct Work {
    const uint8_t* bad;         // per clique: the host's vertex range test failed
    const Owner* own;           // the owners' list
    uint64_t n_own;
    uint64_t *key_in, *key;     // per item: clique << 32 | vertex, as given and sorted
    uint32_t* m_item;           // per member: where its vertex lies in key (kNone: not the first layout of an owner, or no clique vertex)
    uint32_t* m_owner;          // per member: index into own, or kNone
    uint64_t *m_cnt, *m_off;    // per member: member_items of an owned member, and the exclusive sum (n_members + 1)
    uint32_t* sr_of;            // per clique: its place among the surviving super-reads, or kNone
    uint64_t *sub_cnt, *pre_cnt, *pre_off;  // per super-read (+ 1): clique vertices; index entries of a self-merged one, else 0; its sum
    uint64_t *it_key_in, *it_key;           // the index entries in pre-order and sorted
    uint32_t *it_val_in, *it_val;           // their vertices
};
// the tables in device memory, as hc_sr_clique_next_output names them: mn::Tables with pair_kind = clique_kind, pair_new_id =
// clique_new_id, sr_pair = sr_clique, clique_cnt / clique_off the rows' sizes and offsets, subread_off the second CSR's offsets

// hc_sr_clique_next_kernels.hip; every launch is one kernel whatever the sizes
hipError_t launch_items(In I, Work W, hipStream_t stream);                // key_in
hipError_t launch_cliques(In I, Work W, mn::Slots S, hipStream_t stream);  // the cliques' entries
hipError_t launch_members(In I, Work W, hipStream_t stream);               // m_owner, m_item, m_cnt (after the sort of the keys)
hipError_t launch_mark(In I, Work W, mn::Slots S, hipStream_t stream);     // after the check: visited, lane per member
hipError_t launch_keys(In I, mn::Slots S, hipStream_t stream);             // after the check: the cliques' terms of the rank sum
// after the rank sum: the surviving cliques' entries to their places, ids, kinds, srs, sr_clique, the sizes of the three per-super-read lists
hipError_t launch_order(In I, Work W, mn::Slots S, mn::Totals N, hc_sr_next_entry* out_entries, uint32_t* out_status, uint64_t* out_cnt,
                        uint64_t* out_bytes, mn::Tables T, hipStream_t stream);
// after the sums of the sizes: the plain rows, the self-merged cliques' index entries in pre-order (lane per member); the subread table
// (lane per item); the self-merged rows from the sorted entries (lane per entry)
hipError_t launch_member_rows(In I, Work W, mn::Slots S, mn::Tables T, hipStream_t stream);
hipError_t launch_subreads(In I, Work W, mn::Slots S, mn::Tables T, hipStream_t stream);
hipError_t launch_merged_rows(Work W, uint64_t n_entries, mn::Tables T, hipStream_t stream);

}  // namespace cn
}  // namespace hc
