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

}  // namespace hc
