// hc_br.h — the device side of hc_br_evidence (include/hcsr.h): the arrays of one call and the launch interface of hc_br_kernels.hip.
// The width-dependent expressions of the reference are host/BranchEvidence.h's, shared with the host mirror.  Internal: not part of the ABI.
//
// Indices.  A BRANCH b: in-branches in ascending vertex (b < n_in), then out-branches.  A SLOT s: neighbour i of branch b at nb_off[b] + i,
// neighbours ascending.  A PAIR p: pair (i, j), i < j, of branch b at pair_off[b] + i k - i (i + 1) / 2 + (j - i - 1), k neighbours.  A RECORD:
// an index into the graph's edge array, which is in target order: ascending record = ascending (u, v).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcsr.h"
#include "host/BranchEvidence.h"

namespace hc {
namespace br {

// what a pair's wave found (Work::pr_info)
constexpr uint32_t kPairIdentical = 1u;   // no difference: a missing edge and a false mark (:475, :629)
constexpr uint32_t kPairMissing = 2u;     // a missing inclusion pair (:450, :462) ...
constexpr uint32_t kPairMissingI = 4u;    // ... whose node_pair.first is neighbour i (else j)
constexpr uint32_t kPairFailShift = 8u;   // HC_BR_* << 8: the assert this pair fails
// counters (Work::counters)
enum { kCntDiffSel = 0, kCntNbSel, kCntEvSel, kCntRecSel, kCntMissSel, kCntArgError, kCntBadOriginal, kCounters = 8 };

struct Graph {
    const hc_edge_rec* edges;  // in target order
    const uint64_t* out_off;
    const uint32_t* in_nodes;
    const uint64_t* in_off;
    uint32_t V, E;
};
struct Store {  // the kept raw arrays of the current store
    const uint8_t* bases;
    const uint64_t* off;     // n_seq + 1
    const uint32_t* first;   // n_reads + 1
    uint32_t n_reads;
};
struct Dict {
    const uint64_t* off;
    const hc_sr_original* entries;
};
struct Originals {
    const uint8_t* bases;
    const uint64_t* off;
    uint64_t n;
};
struct In {
    Graph g;
    Store st;
    Dict d;
    Originals o;
    const uint32_t* vread;
    const uint8_t* vfwd;
    uint64_t se, pe, orc;
    uint32_t min_overlap_len;
    double edge_threshold;
};

struct Work {
    // per vertex and side (2 V + 1), each with its exclusive sum in place: branches, neighbours, pairs
    uint64_t *cnt_b, *cnt_s, *cnt_p;
    // adj_in as owner << 32 | source, and sorted (sortAdjLists, :47)
    uint64_t *in_key_a, *in_key_b;
    // per record: stored from its in-branch / its out-branch / either; the listed records
    uint8_t *rec_in, *rec_out, *rec_flag;
    uint32_t* rec_sel;
    // per branch (n_b, the offsets n_b + 1)
    uint64_t n_b, n_in, n_s, n_p;
    uint32_t* br_node;
    uint64_t *nb_off, *pair_off, *diff_off;
    uint32_t *br_status, *br_node1len;
    int32_t* br_dist;
    uint8_t *br_false, *br_status8;
    // per slot (n_s; sl_items n_s + 1 with its exclusive sum in sl_item_off)
    uint32_t *sl_node, *sl_rec, *sl_len, *sl_olen, *nb_sel;
    int32_t *sl_pos, *sl_start;
    uint64_t *sl_seq, *sl_items, *sl_item_off;
    uint8_t *sl_paired, *sl_keep;
    // per pair (n_p; pr_cnt n_p + 1 with its exclusive sum in pr_off; pr_diff: HC_BR_MAX_DIFFS slots each)
    uint32_t *pr_raw, *pr_cnt, *pr_off, *pr_info, *miss_sel;
    int32_t *pr_term, *pr_rel, *pr_len, *pr_diff;
    uint8_t* pr_miss;
    // per diff slot in use (n_d)
    uint64_t *dk_in, *dk;
    uint8_t* d_flag;
    uint32_t *d_sel, *d_branch;
    // per item key (2 n_items)
    uint64_t *ek_in, *ek;
    uint8_t* e_flag;
    uint32_t *e_sel, *e_rec;
    unsigned long long* counters;
    // the tables
    hc_br_branch* t_branches;
    uint32_t* t_nb;
    int32_t* t_diff;
    uint32_t* t_ev_edge;
    uint64_t* t_ev_off;
    uint32_t* t_ev_ids;
    hc_edge_rec* t_missing;
};

// A
hipError_t launch_count(const In& I, const Work& W, hipStream_t s);                    // 2 V + 1 lanes
hipError_t launch_in_keys(const In& I, const Work& W, hipStream_t s);                  // E lanes
hipError_t launch_branches(const In& I, const Work& W, hipStream_t s);                 // 2 V + 1 lanes
hipError_t launch_slots(const In& I, const Work& W, hipStream_t s);                    // n_s lanes
hipError_t launch_branch_geometry(const In& I, const Work& W, hipStream_t s);          // n_b lanes
hipError_t launch_pairs(const In& I, const Work& W, hipStream_t s);                    // n_p waves
// B
hipError_t launch_branch_verdict(const In& I, const Work& W, hipStream_t s);           // n_b lanes
hipError_t launch_diff_keys(const Work& W, uint64_t n_d, hipStream_t s);
hipError_t launch_diff_first(const Work& W, uint64_t n_d, hipStream_t s);
hipError_t launch_diff_gather(const Work& W, uint64_t n_d, hipStream_t s);
hipError_t launch_diff_offsets(const Work& W, hipStream_t s);                          // n_b + 1 lanes
hipError_t launch_nb_gather(const Work& W, hipStream_t s);                             // n_s lanes
// C
hipError_t launch_items(const In& I, const Work& W, uint64_t n_items, hipStream_t s);
// D
hipError_t launch_record_flags(const Work& W, hipStream_t s);                          // n_s lanes
hipError_t launch_ev_keep(const In& I, const Work& W, uint64_t n_keys, hipStream_t s);
hipError_t launch_ev_gather(const Work& W, uint64_t n_keys, hipStream_t s);
hipError_t launch_ev_edges(const In& I, const Work& W, hipStream_t s);                 // E + 1 lanes
hipError_t launch_missing(const In& I, const Work& W, hipStream_t s);                  // n_p lanes
hipError_t launch_assemble(const Work& W, hipStream_t s);                              // n_b lanes


// ---- hc_br_reduce (hc_br_reduce_kernels.hip) --------------------------------------------------------------------------------------------
// A COMPONENT EDGE e: edge k of component c at cm_first[c] + k (the host's CSR of branching_components).  An ITEM i: id k of component edge
// e at ce_off[e] + k.  A ROW: an edge of the evidence tables (t_ev_edge, ascending (u, v)).
enum { kRedBadRead = 0, kRedBadId, kRedNotFound, kRedCounters = 4 };
constexpr uint32_t kNoRow = 0xffffffffu;

struct Red {
    // per final_branch neighbour (n_nb): the slot it was gathered from, its record; out: len1, len2, overlap len0
    const uint32_t *nb_sel, *sl_rec;
    int32_t* tri;
    uint64_t n_nb;
    // the evidence tables
    const uint32_t* ev_edge;
    const uint64_t* ev_off;
    const uint32_t* ev_ids;
    uint64_t n_rows;
    // per component edge (n_ce; ce_len n_ce + 1 with its exclusive sum in ce_off)
    uint32_t *ce_u, *ce_v, *ce_comp, *ce_row, *ce_count;
    uint64_t *ce_len, *ce_off;
    uint8_t* ce_remove;
    uint64_t n_ce;
    // per component (n_c; cm_first n_c + 1)
    uint64_t* cm_first;
    int32_t* cm_minev;
    uint8_t *cm_no_row, *cm_keep;
    uint64_t n_c;
    // per item (n_items; uniq n_items + 1, summed in place)
    uint64_t *key_in, *key, *uniq;
    uint32_t *val_in, *val;
    uint64_t n_items, id_limit;  // id_limit = 2 * original_readcount: every id is below it
    int id_bits;
    // per removed pair (n_rm): out: its record and its adj_in entry
    uint32_t *rm_u, *rm_v, *rm_rec, *rm_in;
    uint64_t n_rm;
    unsigned long long* counters;
};

hipError_t launch_red_triples(const Graph& g, const Store& st, const Red& R, hipStream_t s);  // n_nb lanes
hipError_t launch_red_rows(const Red& R, hipStream_t s);                                     // n_ce lanes
hipError_t launch_red_keys(const Red& R, hipStream_t s);                                     // n_items lanes
hipError_t launch_red_unique(const Red& R, hipStream_t s);                                   // n_items lanes
hipError_t launch_red_counts(const Red& R, hipStream_t s);                                   // n_ce lanes
hipError_t launch_red_decide(const Red& R, hipStream_t s);                                   // n_c lanes
hipError_t launch_red_find(const Graph& g, const Red& R, hipStream_t s);                     // n_rm waves

}  // namespace br
}  // namespace hc
