// hc_sr.h — what the super-read consensus kernels (hc_sr_kernels.hip) and their glue (hc_api_sr.cpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hcsr.h"
#include "hc_device.h"

namespace hc {

// (the tables' geometry, the entry codes and the safe region: host/SrCodes.h.  The store's quality indices are term indices as they
// stand: K + 2 <= 97, wide labels < 64, both below sr::kQDim)
constexpr uint32_t kSrLateBadSymbol = 1u, kSrLateNaN = 2u;  // what a column reports about its layout

struct SrMember {  // a member resolved against the store
    uint64_t off;  // first symbol of the oriented sequence
    uint32_t len;
    int32_t pos;
};
static_assert(sizeof(SrMember) == 16, "SrMember is 16 bytes");

struct SrLayoutInfo {
    int32_t ret;      // what consensus() returns
    uint32_t status;  // HC_SR_*
    uint32_t len;     // columns written
    int32_t trim;     // trim_pos: the first column
};

struct SrHostColumn {  // a column the host finishes (:348-396) from the device's sums
    uint64_t out;      // its place in the packed buffers
    uint32_t n;        // nucleotides.length()
    uint32_t layout;
    double s[4];       // by base code A, C, G, T
};
static_assert(sizeof(SrHostColumn) == 48, "SrHostColumn is 48 bytes");

hipError_t sr_launch_layouts(const StoreView& st, const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members, uint64_t n_members,
                             uint32_t minimum_support, uint32_t error_correction, SrMember* mem, SrLayoutInfo* info, uint64_t* out_len,
                             hipStream_t s);
hipError_t sr_launch_columns(const StoreView& st, uint32_t n_cu, const hc_sr_layout* layouts, uint64_t n_layouts, const SrMember* mem,
                             const SrLayoutInfo* info, const uint64_t* out_off, const double* terms, const uint8_t* qbyte, const uint8_t* table,
                             uint32_t safe_region, uint8_t* cons_seq, uint8_t* cons_qual, uint32_t* late, SrHostColumn* host_cols,
                             uint64_t host_cap, unsigned long long* host_count, hipStream_t s);

// hc_sr_edge_kernels.hip: the edge merge (hc_sr_edge_merge, hc_graph_merge_pairs).  A pair owns two layout slots and six member slots
// until the counts are summed; `who` says which of the pair's sorted vertices (0 / 1) a member slot belongs to.
struct SrEdgeSlots {
    uint32_t* status;         // [n_pairs] HC_SR_EDGE_*
    uint64_t* lay_cnt;        // [n_pairs + 1] layouts of the pair, the last entry 0
    uint64_t* mem_cnt;        // [n_pairs + 1] members of the pair
    hc_sr_layout* layouts;    // [2 n_pairs] first_member: unset
    hc_sr_member* members;    // [6 n_pairs] members of slot k at 3 k
    uint8_t* who;             // [6 n_pairs]
};
hipError_t sr_edge_launch_targets(const hc_edge_rec* edges, uint64_t n_edges, uint32_t* targets, hipStream_t s);
hipError_t sr_edge_launch_layouts(const StoreView& st, const hc_edge_rec* edges, const unsigned long long* out_off, uint64_t n_vertices,
                                  const uint32_t* pairs, uint64_t n_pairs, const uint32_t* vertex_read, const uint8_t* vertex_fwd, SrEdgeSlots slots,
                                  hipStream_t s);
hipError_t sr_edge_launch_compact(SrEdgeSlots slots, uint64_t n_pairs, const uint64_t* first_layout, const uint64_t* mem_off, hc_sr_layout* layouts,
                                  hc_sr_member* members, hipStream_t s);
hipError_t sr_edge_launch_subreads(SrEdgeSlots slots, uint64_t n_pairs, const uint64_t* first_layout, const SrLayoutInfo* info,
                                   hc_sr_subread_info* subreads, hipStream_t s);

// hc_sr_clique_kernels.hip: cliques of any size (hc_sr_clique_merge).  An ITEM is one (clique, vertex) of the call in (clique, vertex)
// order; it owns two entry SLOTS (2 j, 2 j + 1): mate 1 / mate 2 of a paired read in an 's' layout, the 'l' / the 'r' entry in a 'p'
// clique.  A PROVISIONAL LAYOUT (pl) is a layout of a clique that passed the range checks, numbered before the loop's and the
// geometry's verdicts are known; an ENTRY index i counts the entries of all provisional layouts in list order.
struct SrCliqueSlot {
    int64_t pos[2];  // before the shift
    uint32_t len[2];
    hc_sr_member m[2];
    uint32_t n, pad;
};
struct SrCliquePl {
    uint64_t start;  // first entry
    uint32_t n;      // entries
    uint32_t clique;
    uint32_t which;  // 0: 's' or 'l', 1: 'r'
    uint32_t base_len;
};
struct SrCliqueView {
    // the call's inputs
    uint64_t C, N, V;
    const uint64_t* off;        // [C + 1]
    const uint32_t* vread;      // [V]
    const uint8_t* vfwd;        // [V]
    const hc_edge_rec* E;
    const unsigned long long* out_off;
    uint32_t m;                 // min_clique_size
    // per item, in sorted order
    uint64_t* key;              // [N] clique << 32 | vertex
    uint32_t* hit;              // [N] first base -> node record in list order, or none
    SrCliqueSlot* slot;         // [N]
    uint64_t* ecnt;             // [N + 1] entries of the item
    uint64_t* eoff;             // [N + 1] their exclusive sum
    uint32_t* sel;              // [2 N] filter_subreads' selected_nodes, per item and layout
    hc_sr_subread_info* sub;    // [N]
    // per clique
    unsigned long long* failkey;  // rank << 8 | status of the first failing vertex, ~0: none
    uint32_t* base_rank;
    uint8_t* type;                // 's' | 'p'
    uint32_t* geom;               // an assert behind the loop failed
    unsigned long long* ext;      // [4 C] l_ext, r_ext of layout 0 and 1
    uint64_t* deg;                // [C + 1] records of the base's list; rec_off: their exclusive sum
    uint64_t* rec_off;
    uint64_t* lay0;               // [C + 1] provisional layouts; pl_first: their exclusive sum
    uint64_t* pl_first;
    uint32_t* status;             // [C]
    uint64_t* lay_cnt;            // [C + 1] final; first: exclusive sum
    uint64_t* first;
    uint64_t* mem_cnt;            // [C + 1] final; mem_off: exclusive sum
    uint64_t* mem_off;
    // per provisional layout
    SrCliquePl* pl;
    int32_t* pl_total;
    uint8_t* pl_filter;           // HC_SR_FILTER_*
    // per entry: sort input and output of the list order, then of the endpos order
    uint64_t* ekey_in;
    uint64_t* ekey;
    uint32_t* eval_in;
    uint32_t* eval;               // slot of entry i
    uint32_t* slotpos;            // [2 N] entry of a slot
    hc_sr_member* fmem;           // the full lists
    uint32_t* fvert;
    int32_t* fend;                // pos + len
    uint8_t* fused;
    // final order
    hc_sr_layout* out_layouts;
    hc_sr_member* out_members;
    uint32_t* out_vertex;
    uint8_t* out_used;
    uint8_t* out_filter;
    uint64_t* uflag;              // [M + 1]; uoff: exclusive sum
    uint64_t* uoff;
};
hipError_t sr_clique_launch_keys(const SrCliqueView& W, const uint32_t* nodes, uint64_t* key_in, hipStream_t s);
hipError_t sr_clique_launch_precheck(const StoreView& st, const SrCliqueView& W, hipStream_t s);
hipError_t sr_clique_launch_bases(const SrCliqueView& W, hipStream_t s);
hipError_t sr_clique_launch_hits(const SrCliqueView& W, uint64_t n_records, hipStream_t s);
hipError_t sr_clique_launch_nodes(const StoreView& st, const SrCliqueView& W, hipStream_t s);
hipError_t sr_clique_launch_entries(const SrCliqueView& W, hipStream_t s);
hipError_t sr_clique_launch_geometry(const SrCliqueView& W, uint64_t n_entries, hipStream_t s);
hipError_t sr_clique_launch_filter(const SrCliqueView& W, uint64_t n_pl, const uint64_t* ekey2, const uint32_t* eval2, hipStream_t s);
hipError_t sr_clique_launch_status(const SrCliqueView& W, hipStream_t s);
hipError_t sr_clique_launch_compact(const SrCliqueView& W, uint64_t n_entries, hipStream_t s);
hipError_t sr_clique_launch_consensus_input(const SrCliqueView& W, uint64_t n_layouts, uint64_t n_members, hc_sr_layout* layouts, hc_sr_member* members,
                                            hipStream_t s);
hipError_t sr_clique_launch_subreads(const SrCliqueView& W, const SrLayoutInfo* info, hipStream_t s);

}  // namespace hc
