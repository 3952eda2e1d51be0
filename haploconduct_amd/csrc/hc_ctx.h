// hc_ctx.h — the context behind the C ABI (include/hcedge.h), shared by the hc_api*.cpp translation units, and the
// launch interface of the kernel translation units.  Internal: nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <utility>
#include <string>
#include <vector>

#include "../../include/hcedge.h"
#include "../../include/hcsr.h"
#include "hc_device.h"
#include "hc_overlap_finder.h"
#include "hc_scratch.h"

namespace hc {
// hc_kernels.hip
hipError_t launch_encode(uint32_t symbytes, const uint8_t* bases, const uint8_t* quals, const uint64_t* raw_off,
                         const uint64_t* seq_off, const uint32_t* rc_delta, const uint8_t* qmap, uint32_t n_seq, uint32_t K, void* sym,
                         uint8_t* seq_bad, const uint32_t* read_first_seq, uint32_t n_reads, ReadDesc* descs, uint32_t slot_align,
                         hipStream_t stream);
// The scoring launch: plan_score_launch decides all of it (no HIP call in it), launch_score carries the plan out.
// One row of the table of compiled scoring kernels (hc_kernels.hip); the first eight fields are the key.
struct ScoreKernel {
    bool coop;                  // score_kernel_coop; otherwise score_kernel (256 lanes) or score_kernel_wide_wg (512)
    uint32_t symbytes, lg, wg;  // lg: the template's LG (5 for 16-bit symbols)
    uint32_t group;             // per lane: G, 16-symbol chunks per fetch group
    bool bal;                   // per lane: BAL; cooperative: DYN (the length-bucketed launch)
    uint32_t depth;             // cooperative: DEPTH (0: the LDS-DMA form)
    bool wq;                    // cooperative: WQ (the waves take their items by ticket)
    const void* fn;
    const char* name;           // as hc_get_kernel_info reports it
};
// segmented: rows that may collect in per-workgroup segments (hc_score_pack_device); unsegmented: rows appended straight to the payload
// (a text block's lines travel with them, or a payload of 2^32 rows and more)
enum class RowSinkKind { none, segmented, unsegmented };
struct ScorePlan {
    const ScoreKernel* kernel = nullptr;  // nullptr: the table has no kernel for the plan (a bug)
    const ScoreKernel* staged = nullptr;  // cooperative: the register-staged form, which launches below the LDS-DMA threshold take
    uint32_t blocks = 0;
    size_t lds = 0;           // dynamic LDS per workgroup; more than lds_form when it keeps further workgroups off the CU
    size_t lds_form = 0;
    uint32_t waves_per_cu = 0;
    bool bucketed = false;    // bucket_perm_kernel runs first (scratch: ScoreBuffers::bucket_perm / bucket_queue)
    bool segmented = false;   // the rows collect in per-workgroup segments (scratch: ScoreBuffers::seg_* / spill_turn)
};
// coop_fetch: the cooperative fetch where the store and the table allow it; lane_group: the per-lane kernel's fetch groups otherwise (4 =
// 64-symbol groups for short reads, 2 = 32-symbol groups for contig-length sequences), chosen per read set by hc_set_reads.
ScorePlan plan_score_launch(const StoreView& st, bool coop_fetch, int lane_group, uint32_t n_cu, uint64_t n, RowSinkKind sink);
struct ScoreBuffers {
    // rows == nullptr: plain scoring; otherwise every non-dropped record is also appended to rows (hc_kernels.hip: RowSink)
    hc_gather_row* rows = nullptr;
    unsigned long long* row_count = nullptr;
    uint64_t cap = 0, base_index = 0;
    const hc_line_rec* lines_in = nullptr;
    hc_line_rec* lines_out = nullptr;
    // bucket_perm (n uint32) / bucket_queue (one uint32): scratch of the length-bucketed launch
    uint32_t* bucket_perm = nullptr;
    uint32_t* bucket_queue = nullptr;
    // seg_buf (seg_total_rows rows: segments, then `cap` rows of spill area) / seg_count (kSinkMaxGroups counters + 2 spill counters, all
    // zero before the first launch) / spill_turn (host: which spill counter the next launch uses; advanced by a launch that used segments)
    hc_gather_row* seg_buf = nullptr;
    uint32_t* seg_count = nullptr;
    uint64_t seg_total_rows = 0;
    uint32_t* spill_turn = nullptr;
    // hc_comm_gate_device: the cooperative launch's workgroups add one each to *started as they start
    unsigned long long* started = nullptr;
};
// *started_groups = how many workgroups add to ScoreBuffers::started (0: the launch took a kernel that does not count)
hipError_t launch_score(const ScorePlan& plan, const StoreView& st, ScoreParams prm, const double* lut_g, const void* in, uint64_t n,
                        hc_result_rec* out, const uint32_t* perm, const ScoreBuffers& buf, hipStream_t stream, uint32_t* started_groups);
hipError_t set_score_kernel_lds_limit();
std::string describe_score_kernel(const StoreView& st, bool coop_fetch, int lane_group, uint32_t n_cu, uint64_t n);  // n == 0: the forms in general
// hc_util_kernels.hip
size_t compact_temp_bytes(uint32_t n);
hipError_t launch_compact(const hc_result_rec* res, uint32_t n, uint32_t* idx_out, unsigned long long* count_out, void* temp,
                          size_t temp_bytes, hipStream_t stream);
hipError_t launch_narrow_payload(const void* in32, uint64_t cap, void* out24, uint32_t n_cu, hipStream_t stream);
hipError_t launch_pack_rows(const hc_result_rec* res, const uint32_t* idx, const unsigned long long* count, uint64_t cap, uint64_t base,
                            hc_gather_row* rows, uint32_t n_cu, hipStream_t stream);
hipError_t launch_pack_header(const unsigned long long* count, hc_gather_row* header, hipStream_t stream);
hipError_t launch_gather_results(const hc_result_rec* res, const uint32_t* idx, const unsigned long long* count,
                                 hc_result_rec* out, uint32_t n_cu, hipStream_t stream);
size_t reorder_temp_bytes(uint32_t n);
hipError_t launch_reorder(uint32_t n_reads, uint32_t fmt, const void* in, uint32_t n, uint32_t* keys_in, uint32_t* keys_out,
                          uint32_t* idx_in, uint32_t* perm_out, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_count_positions(const StoreView& st, uint32_t min_read_len, uint32_t fmt, const void* in, uint64_t n,
                                  unsigned long long* totals, hipStream_t stream);
hipError_t launch_kept_rows(const hc_result_rec* res, uint64_t n, const unsigned long long* n_dev, uint64_t base_index, uint32_t* tile_cnt,
                            uint32_t* tile_off, hc_gather_row* rows, uint64_t cap, unsigned long long* count, const hc_line_rec* lines_in,
                            hc_line_rec* lines_out, hipStream_t stream, const uint32_t* text_tally = nullptr,
                            unsigned long long* text_counters = nullptr);  // (a text block: the parse kernel's tallies are summed on the way)
hipError_t launch_flush_text_rows(const void* rows, void* rows_mapped, const void* lines, void* lines_mapped, const unsigned long long* count,
                                  uint64_t cap, const unsigned long long* counters, unsigned long long* counters_mapped, uint32_t n_cu,
                                  hipStream_t stream);
hipError_t launch_comm_gate(const unsigned long long* started, unsigned long long target, uint32_t timeout_us, hipStream_t stream);
hipError_t launch_flush_rows(const void* src, void* dst_mapped, const unsigned long long* count, uint64_t cap, uint32_t row_bytes, uint32_t n_cu,
                             hipStream_t stream);

// hc_locality.hip: the reads' locality order (hc_set_reads) and a launch's walk of its runs in that order (hc_ctx_score)
size_t locality_order_temp_bytes(uint32_t n_reads);
hipError_t launch_locality_order(const uint8_t* bases, const uint64_t* raw_off, const uint32_t* read_first_seq, uint32_t n_reads, uint64_t* keys_a,
                                 uint64_t* keys_b, uint32_t* idx, uint32_t* order_out, void* temp, size_t temp_bytes, hipStream_t stream);
size_t locality_index_work_words(uint32_t n_reads);
hipError_t launch_locality_index(const uint32_t* order, uint32_t n_reads, const void* in, uint64_t n, const unsigned long long* n_dev, uint32_t* bounds,
                                 uint32_t* work, uint32_t* flag, uint32_t* perm, hipStream_t stream);

// hc_api.cpp: the x-space image of a score threshold with a guard band of 2^log2_width relative width (-49: the scoring path's), and the
// log-probability table of the scoring path in its 16-bit-symbol layout (hc_device.h: two triangles of (K + 2) rows) for the Phred values
// `phred`; false: the table is not symmetric in the two qualities
Band threshold_band(double T, int log2_width);
// hc_api.cpp: hc_set_reads in parts, for the calls that replace the store from raw arrays that are on the device already
// (hc_api_sr_next.cpp).  hc_set_reads = its own checks, histograms and copies + plan_store + release_store + finish_store.
struct StorePlan {
    std::vector<uint32_t> seq_len;  // in: the sequences' lengths (one entry at least)
    uint64_t total = 0;             // in: their sum
    uint8_t qmap[256];              // quality byte -> quality index as the symbols carry it, 255: not a quality value of the set
    uint32_t K = 0, symbytes = 0, slot_align = 0;
    uint64_t nsym = 0;
    std::vector<uint64_t> sym_off;
    std::vector<uint32_t> rc_delta;
    std::vector<double> lut;
    bool any_bad_base = false;
};
}  // namespace hc
struct hc_ctx;
namespace hc {
int plan_store(hc_ctx* c, const uint64_t* hist, const uint64_t* base_hist, const uint32_t* read_first_seq, uint32_t n_reads, StorePlan& P);
void release_store(hc_ctx* c);
int finish_store(hc_ctx* c, const StorePlan& P, const uint8_t* d_bases, const uint8_t* d_quals, const uint64_t* d_raw_off, const uint32_t* d_first,
                 const uint32_t* read_first_seq, uint32_t n_reads);
bool build_log_table_u16(const std::vector<int>& phred, double mismatch_setting, std::vector<double>& lut);
}  // namespace hc

// Scratch of one length-bucketed scoring launch (hc::bucket_perm_kernel): the queue counter, then the permutation.  One per
// thing that launches on its own stream (the context, every hc_block / hc_textblock); grow-only.
struct hc_bucket_ws {
    hc_scratch mem;
    int ensure(uint64_t n) { return mem.ensure((n + 16) * sizeof(uint32_t)); }
    uint32_t* queue() const { return mem.as<uint32_t>(); }
    uint32_t* perm() const { return mem.as<uint32_t>() + 16; }
};

struct hc_ctx {
    hc_settings settings;
    int device = 0;
    uint32_t n_cu = 256;
    bool coop_fetch = true;  // the scoring kernel fetches symbols cooperatively (quads read 64-byte rows; stores below 4 GiB)
    int fetch_group = 4;     // otherwise per lane, in groups of 4 (short reads) or 2 (contigs, 16-bit symbols) 16-symbol chunks;
                             // chosen per read set in hc_set_reads (HC_FETCH_GROUP=coop|4|2 overrides: a tuning knob only)
    hipStream_t stream = nullptr;
    hipStream_t text_copy_stream[4] = {nullptr, nullptr, nullptr, nullptr};  // the text blocks' host-to-device copies, in turn (hc_api_text.cpp)
    std::atomic<uint32_t> text_copy_next{0};  // (the streams themselves are created by the one thread that submits: hcedge.h)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // read store
    bool have_reads = false;
    hc_scratch d_sym, d_reads, d_lut, d_inv_n;  // symbols, hc::ReadDesc per read, the log-probability table, StoreView::inv_n
    uint32_t len_p5 = 0, len_p95 = 0;  // 5th / 95th percentile of the sequence lengths: what the kernel dispatch calls "mixed"
    uint64_t store_bytes = 0;
    hc::StoreView view{};
    hc::ScoreParams params{};
    // what the overlap finder needs of the sequences (host copies, filled by hc_set_reads)
    std::vector<hc::SeqRef> seq_refs;  // by store sequence index
    bool singles_first = true;
    // Grow-only device scratch of the finder, one slot per buffer, and of the SFO ingest (hc_found_to_overlaps).  Like d_found and
    // d_found_lines it outlives the read store (hc_set_reads, hc_reset) and goes with the context: gigabytes at config 3's size, and
    // giving them back and asking for them again stalled the next stage's first kernels by 0.3 - 0.4 s (profiles/r06_stage_a_from_store.md).
    hc_scratch finder_scratch[24], ingest_scratch[12];
    hc_scratch h_ingest[2] = {hc_scratch(hipHostMallocDefault), hc_scratch(hipHostMallocDefault)};  // page-locked ring hc_found_to_overlaps copies the sorted records through
    hc_scratch h_sfo_text[3] = {hc_scratch(hipHostMallocDefault), hc_scratch(hipHostMallocDefault),
                                hc_scratch(hipHostMallocDefault)};  // page-locked stations of hc_set_found_from_sfo_text (32 MiB + 64 each), kept
    // result of the last hc_find_overlaps, kept on the device so that the usual "ask for the count, then fetch"
    // pair of calls computes once
    hc_scratch d_found;  // hc_sfo_rec, grow-only (round 6): n_found of them valid
    uint64_t n_found = 0;
    hc_scratch d_found_lines;  // hc_line_rec, hc_found_to_lines_device: the overlap lines of the found records, kept until the next call
    double found_err = -1;
    uint32_t found_min = 0, found_flags = 0;
    bool found_valid = false;
    // grow-only workspace for the host-buffer entry points
    hc_scratch d_in, d_out;  // hc_overlap_rec / hc_result_rec, as many of each
    hc_scratch d_totals;     // two unsigned long long
    // candidate reorder (HC_REORDER_*): scratch for the (key, index) radix sort, grow-only
    int reorder_mode = HC_REORDER_AUTO;
    hc_scratch d_sort, d_sort_tmp;  // d_sort: 4 arrays of as many uint32 each (keys_in, keys_out, idx_in, perm)
    hc_bucket_ws bucket;  // length-bucketed launches on the context's own entry points
    // locality order (hc_locality.hip): the reads sorted by the minimiser of mate /1, built by hc_set_reads for a regular store and kept with
    // it; the per-launch scratch (flag, run boundaries and starts, the launch's permutation) is grow-only and shares `scratch_done`
    hc_scratch loc_order, loc_ws, loc_tmp;
    uint32_t loc_reads = 0;  // reads loc_order holds (0: no order for this read set)
    hc_scratch sink_rows, sink_counts;  // hc_score_pack_device: the row sink's per-workgroup segments (hc_kernels.hip: RowSink)
    uint32_t sink_turn = 0;             // which of the two spill counters the next segmented launch uses
    bool sink_dirty = false;            // a segmented launch failed at enqueue: the spill counters are re-zeroed before the next one
    // the multi-GPU step (hc_set_comm_reserve / hc_comm_gate_device): CUs left free for the collective library's kernels, and the
    // count of workgroups that have started, which the gate kernel on the exchange's stream waits for
    uint32_t comm_reserve = 0;
    hc_scratch d_started;  // one unsigned long long
    unsigned long long started_target = 0;  // workgroups launched so far with the counter (host side)

    // The context's own scratch (reorder workspace, `bucket`, the sink's segments) serves one launch at a time: a launch that uses
    // any of it on another stream than the last such launch waits for that one (hc_ctx_score)
    hipEvent_t scratch_done = nullptr;
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;
    // compaction scratch, grow-only
    hc_scratch d_compact_tmp, d_compact_idx, d_compact_res;  // idx: uint32, res: hc_result_rec, as many of each
    // hc_text_set_ids (hc_api_text.cpp): FastqStorage::m_ID_to_index on the device
    hc_scratch id_table, id_keys;
    uint64_t id_size = 0;
    int id_shift = 0, id_direct = 1;
    bool have_ids = false;
    // hc_graph_resolve / hc_graph_fetch (hc_api_stage.cpp): device-resident result of the last resolve
    struct Graph {
        hc_scratch adm, E, key0, key1, idx0, idx1, keep, incl, tied, counters, surv, k32a, k32b, k64a, k64b, tmp_idx, o_out, o_in,
            out_off, in_off, edges_out, in_nodes, vtx, temp, tied_list;
        // graph cleaning (hc_graph_remove_inclusions / hc_graph_remove_transitive): the cleaned graph is written into
        // the *_next buffers, which then trade places with the current ones; the inclusion groups stay for fetching
        hc_scratch edges_next, seq_next, out_off_next, in_nodes_next, in_off_next, clean_temp, incl_vtx, incl_off, incl_edges;
        uint64_t n_groups = 0, n_group_edges = 0;
        bool have_groups = false;
        // hc_graph_remove_tips / hc_graph_remove_branches: OverlapGraph::branching_edges (n_branching records) and the per-read
        // tip flags (n_tip_reads bytes), both until the next hc_graph_load / hc_graph_resolve; the read table of one call
        hc_scratch branching, tip_reads, read_geom;
        uint64_t n_branching = 0, n_tip_reads = 0;
        uint64_t n_vertices = 0, n_edges = 0, n_tied = 0;
        uint64_t n_appended = 0;  // records hc_graph_append has put into adm
        uint64_t edits = 0;       // cleaning calls that replaced the lists (what hc_br_reduce checks its tables against)
        uint64_t sorted_at = ~0ull;  // `edits` when hc_graph_sort_edges left its order (hc_graph_remove_cycles' stamp); ~0: never
        bool valid = false;
        // hc_graph_append copies through two page-locked buffers on the context's stream and does not wait for the copy
        hc_scratch h_stage[2] = {hc_scratch(hipHostMallocDefault), hc_scratch(hipHostMallocDefault)};
        hipEvent_t stage_free[2] = {nullptr, nullptr};
        int stage_turn = 0;
    } graph;
    // hc_graph_write_text / hc_graph_text_fetch (hc_api_graph_text.cpp): grow-only scratch — the items' byte counts (their exclusive sum
    // after the scan), the records' keep bytes, the counters, the scan's workspace — and the text itself, n_bytes of it, kept until
    // the next hc_graph_write_text or the next call that replaces or cleans the graph (drop())
    struct GraphText {
        hc_scratch sizes, keep, counters, temp, text;
        uint64_t n_bytes = 0;
        bool valid = false;
        void drop() { valid = false, n_bytes = 0; }
    } graph_text;
    // hc_graph_cliques / hc_graph_cliques_fetch (hc_api_cliques.cpp): grow-only scratch — the pair keys and the rank keys (two blocks
    // each, the sorts' in and out), the simple adjacency (off, nbr, rank, order, kind), the roots' counts and their sums, the counters,
    // the prims' workspace, the waves' slices — and the CSR, kept until the next hc_graph_cliques or the next call that replaces or
    // edits the graph (drop())
    struct Cliques {
        hc_scratch keys_a, keys_b, rank_a, rank_b, off, nbr, rank, order, kind, cnt_c, cnt_e, counters, temp, slices, clique_off, clique_nodes;
        uint64_t n_cliques = 0, n_entries = 0;
        bool valid = false;
        void drop() { valid = false, n_cliques = n_entries = 0; }
    } cliques;
    // hc_graph_label_vertices / hc_graph_fetch_orientations (hc_api_label.cpp): grow-only scratch — one block carved into the arrays of
    // hc_label.h: Work, the prims' workspace, the counters — and vertex_orientations, n_orient bytes of them, kept until the next
    // hc_graph_load / hc_graph_resolve (drop())
    struct Label {
        hc_scratch work, temp, counters, orient;
        uint64_t n_orient = 0;
        bool valid = false;
        void drop() { valid = false, n_orient = 0; }
    } label;
    // hc_graph_sort_edges / hc_graph_remove_cycles / hc_graph_fetch_cycle_pairs (hc_api_cycles.cpp): grow-only scratch — one block carved
    // into the per-graph arrays of the sort or of hc_cycles.h: Work, one into those of the compact CSR (sized once its records are
    // counted) and one into the radix form's keys (only for a graph with a list longer than hc_cycles.h: kRankMax), the prims'
    // workspace, the counters, the page-locked blocks the host walks (try 1; the compact CSR's columns) — and the pairs of the last
    // hc_graph_remove_cycles (u << 32 | v, ascending), valid until the graph is replaced
    struct Cycles {
        hc_scratch work, work_sub, work_radix, temp, counters, pin = hc_scratch(hipHostMallocDefault), pin_sub = hc_scratch(hipHostMallocDefault);
        std::vector<uint64_t> pairs;
        bool valid = false;
        void drop() { valid = false, pairs.clear(); }
    } cycles;
    // The consensus tables of one call path on the device (hc_api_sr.cpp: sr_tables): the log10 terms by term index, q_of itself, the
    // table of one- and two-member columns — and what they were built for.
    struct SrTables {
        hc_scratch terms, qbyte, table;
        bool valid = false, has_nan = false;  // has_nan: the table holds a kEntryNaN
        double min_qual = 0;
        uint8_t q_of[128];  // the quality value (byte - 33) of term index i, 255: none
    };
    // super-read consensus (hc_api_sr.cpp).  hc_set_reads keeps the inverse of its quality map: sr_qbyte[i] = quality byte - 33 of the
    // store's quality index i (255: the index is not a quality value).  The tables are rebuilt when the store or min_qual changes.
    uint8_t sr_qbyte[128];
    struct Sr {
        hc_scratch layouts, members, mem, info, len, off, temp, seq, qual, late, host_cols, counter;
        SrTables tables;
        // hc_sr_keep_device: seq / qual hold the last call's bytes in their final form (kept_bytes of them), patched by `patches`;
        // hc_sr_merge_self_overlaps_kept appends to them and hc_sr_kept_load replaces them (hc_api_sr.cpp)
        hc_scratch patches;
        bool kept_valid = false;
        uint64_t kept_bytes = 0;
    } sr;
    // hc_sr_keep_device / hc_sr_set_next_reads (hc_api_sr_next.cpp).  While `keep` is on, the raw arrays of the current store stay on the
    // device (bases, quals, off: n_seq + 1 offsets, first: n_reads + 1) with host copies of the two small ones; a call gathers the next
    // store's into the next_* blocks, which then trade places with them.  The rest is grow-only scratch of one call.
    struct SrNext {
        bool keep = false, raw_valid = false;
        hc_scratch bases, quals, off, first;
        uint64_t total = 0;
        std::vector<uint64_t> h_off;
        std::vector<uint32_t> h_first;
        hc_scratch next_bases, next_quals, next_off, next_first;
        hc_scratch entries, status, cnt, bytes, cnt_off, byte_off, temp, hist, extra_seq, extra_qual;
        // The store the last next-store call READ (hc_sr_fastq_write_text's tips are reads of it).  prev_traded: the call replaced the store,
        // and that store's raw arrays are the next_* blocks it traded, prev_reads / prev_seq / prev_total of them.  Otherwise it is the
        // current store: the call returned HC_SR_NEXT_EMPTY, or none ran since hc_set_reads.  Cleared wherever the next_* blocks are
        // reallocated, overwritten or freed: the start of a gather, hc_set_reads, hc_sr_keep_device(ctx, 0), hc_reset.
        bool prev_traded = false;
        uint32_t prev_reads = 0, prev_seq = 0;
        uint64_t prev_total = 0;
        void prev_clear() { prev_traded = false, prev_reads = prev_seq = 0, prev_total = 0; }
    } srn;
    // hc_set_reads_from_fastq_text / hc_fastq_fetch (hc_api_fastq.cpp): grow-only scratch — the three files' text (singles, paired1,
    // paired2), their newline counts per tile (the counts' exclusive sum after the scan) and line starts; by read the ids, the tokens'
    // spans and the not-plain flags; by sequence the lengths and their sum; the counters; the scan's workspace — and what hc_fastq_fetch
    // hands out, valid from a successful call until the store is replaced or released
    struct Fastq {
        hc_scratch text[3], tiles[3], line_start[3], ids, tok_off, tok_len, not_plain, lens, off, counters, temp, hist;
        uint64_t chunk_bytes = 0;  // hc_fastq_set_chunk_bytes (0: the default)
        std::vector<uint64_t> read_ids, seq_off;
        std::vector<uint32_t> first;
        hc_fastq_counts counts{};
        bool valid = false;
    } fastq;
    // hc_set_sam_records / hc_sam_plan / hc_sam_lines_device (hc_api_sam.cpp): the uploaded records (alignments, records, operations,
    // reference lengths, the references' first records), the plan's workspace (keys, permutation, counts, the sort's and the sum's scratch,
    // the prefix maximum) and what stays of a plan: the records in the script's order, e_j, the windows' starts and the line offsets
    struct Sam {
        hc_scratch alns, recs, ops, ref_len, seg_begin, proc_end;
        hc_scratch keys, keys_out, iota, perm, cnt, temp, pmax, tiles, status, range, stage;
        hc_scratch pos, len, ref, rec, e, lo, off;
        hc_scratch slot[16];  // hc_sam_lines_slot
        uint32_t n_alns = 0, n_recs = 0, n_refs = 0;
        uint64_t n_ops = 0, n_lines = 0, n_candidates = 0, n_window = 0;
        int64_t mol = 0;
        int key_bits = 64;
        bool loaded = false, planned = false;
    } sam;
    // hc_sr_fastq_write_text / hc_sr_fastq_text_fetch (hc_api_sr_fastq.cpp): grow-only scratch — the items' characters (their exclusive
    // sum after the scan), the scan's workspace, the counters, the tips' reads — and the text of the four files in one block, file f at
    // [bound[f], bound[f + 1]), kept until the next hc_sr_fastq_write_text or until raw arrays it was made from are replaced (drop())
    struct SrFastq {
        hc_scratch sizes, temp, counters, tip_reads, text;
        uint64_t bound[5] = {0, 0, 0, 0, 0};
        bool valid = false;
        void drop() { valid = false; }
    } sr_fastq;
    // self-overlap merge (hc_api_sr.cpp: hc_sr_merge_self_overlaps): grow-only scratch; the consensus tables are rebuilt when min_qual or
    // the batch's quality values change (term index = the value itself)
    struct SrSelf {
        hc_scratch seq, qual, pairs, skip, qmap, lut, inv_n, res, len, off, mpos, temp, out_seq, out_qual;
        // hc_sr_merge_self_overlaps_kept: the check kernel's counters; the host-decided pairs' copy records and staging block
        hc_scratch check, segs, stage_seq, stage_qual;
        SrTables tables;
    } sr_self;
    // edge merge (hc_api_sr_edge.cpp: hc_graph_merge_pairs, hc_sr_edge_merge): grow-only scratch — the target column; the call's pairs and
    // vertex tables, the pairs' slots (hc_sr.h: SrEdgeSlots), the two sums and the subread infos
    struct SrEdge {
        hc_scratch targets, pairs, vread, vfwd, status, lay_cnt, mem_cnt, first, mem_off, layouts, members, who, sub, temp;
    } sr_edge;
    // clique merge (hc_api_sr_clique.cpp: hc_sr_clique_merge): grow-only scratch, the blocks of hc_sr.h: SrCliqueView by name, the call's
    // inputs and the scans' and sorts' workspace; filter_on_host: hc_sr_clique_filter_on_host
    struct SrClique {
        hc_scratch off, nodes, vread, vfwd, key_in, key, hit, slot, ecnt, eoff, sel, sub, failkey, base_rank, type, geom, ext, deg, rec_off, lay0,
            pl_first, status, lay_cnt, first, mem_cnt, mem_off, pl, pl_total, pl_filter, ekey_in, ekey, eval_in, eval, ekey2, eval2, slotpos, fmem, fvert, fend,
            fused, out_layouts, out_members, out_vertex, out_used, out_filter, uflag, uoff, temp;
        bool filter_on_host = false;
    } sr_clique;
    // hc_sr_merge_next (hc_api_sr_merge_next.cpp): grow-only scratch — the call's inputs; its slots (hc_sr_merge_next.h: Slots) and the merged
    // pairs' rewrites; the tables before they are copied out (t_*); the scans' workspace
    struct SrMergeNext {
        hc_scratch pairs, pair_status, first_layout, layouts, members, lay_status, out_off, sub, v_read, v_fwd, incl, tip_reads;
        hc_scratch entries, status, cnt, bytes, key, rank, overlap_pos, n_clique, visited, rewrite;
        hc_scratch t_kind, t_id, t_v_state, t_nodes, t_srs, t_sr_pair, t_clique_cnt, t_clique_off, t_clique_nodes, t_sub_off, t_sub, t_tips, temp;
        // hc_fno1_from_graph (HC_FNO1_TABLES_KEPT) reads t_nodes, t_srs, t_clique_off, t_clique_nodes, t_sub_off and t_sub in place: valid from a
        // successful hc_sr_merge_next / hc_sr_clique_next until the start of the next one (which may reallocate them) or hc_reset
        bool tables_valid = false;
        uint64_t tables_vertices = 0, tables_srs = 0, tables_new_read_count = 0;
        void tables_drop() { tables_valid = false, tables_vertices = tables_srs = tables_new_read_count = 0; }
    } sr_mn;
    // hc_sr_clique_next (hc_api_sr_clique_next.cpp): grow-only scratch — the call's inputs, the host's verdicts (bad, own); the blocks of
    // hc_sr_clique_next.h: Work by name; the row and subread sizes before their sums; the sorts' and scans' workspace.  The slots, the
    // rewrites and the tables are sr_mn's: the two calls never run at once on one context.
    struct SrCliqueNext {
        hc_scratch off, nodes, cstatus, first_layout, layouts, mvertex, lay_status, out_off, sub, v_read, v_fwd, bad, own;
        hc_scratch key_in, key, m_item, m_owner, m_cnt, m_off, sr_of, sub_cnt, pre_cnt, pre_off, it_key_in, it_key, it_val_in, it_val, temp;
    } sr_cn;
    // hc_sr_originals_* (hc_api_sr_originals.cpp): the kept dict (off: n_reads + 1 offsets, entries: n_entries hc_sr_original), which
    // hc_sr_originals_next trades against next_off / next_entries; the call's inputs (in_*); the blocks of hc_sr_originals.h: Work by name;
    // the text (sizes: the items' characters and their sum, text: n_text bytes of it, kept until the dict is replaced)
    struct SrOriginals {
        hc_scratch off, entries, next_off, next_entries;
        uint64_t n_reads = 0, n_entries = 0;
        bool valid = false;
        hc_scratch in_kind, in_new_id, in_overlap_pos, in_first_layout, in_layouts, in_sr_clique, in_subread_off, in_subreads, in_vertex_state, in_nodes,
            in_vertex_read, in_vertex_fwd;
        hc_scratch cnt, cnt_off, key_in, key, val_in, val, cand, bits, flag, sel, n_sel, out_id, out_status, temp;
        hc_scratch sizes, text;
        uint64_t n_text = 0;
        bool text_valid = false;
        // hc_fno3_from_originals (hc_api_fno3_resident.cpp): the blocks of hc_fno3_walk.h: Work by name, the walk ranks, the records and
        // lines of fno3_deduce / fno3_format; the text (n_text bytes) and the candidate table (n_cands rows), built in next_* and traded
        // at the end, kept until the dict or the store is replaced
        struct Fno3 {
            hc_scratch key1_in, key1, val1_in, val1, entry_read, head1, head1_pos, cnt, key2_in, key2, val2_in, val2, diff, head2, differs, head2_pos,
                counters, temp, rank, items, rec, len, off;
            hc_scratch text, next_text, cands, next_cands;
            uint64_t n_text = 0, n_cands = 0;
            bool valid = false;
            void drop() { valid = false, n_text = 0, n_cands = 0; }
        } fno3;
        void text_replaced() { text_valid = false, n_text = 0; }
        void replaced() { text_replaced(), fno3.drop(); }
    } sr_orig;
    // hc_fno1_from_graph (hc_api_fno1_resident.cpp): grow-only scratch — the call's inputs (non-edges, caller tables), the flags and
    // selections of checkEdge, the sorted subread maps, and `pool`, the blocks the shared walk (hc_api_fno.cpp: fno1_walk_from_device) takes
    // in the order it asks for them — and what the fetches hand out: the walk's edge list (n_seg: its four segments), the text and the
    // lines, built in next_* and traded at the end, kept until the next call or until the graph or the store is replaced (drop())
    struct Fno1 {
        hc_scratch nonedges, nodes, srs, clique_off, clique_nodes, sub_off, sub, sub_sorted, sub_key_in, sub_key, sub_val_in, sub_val;
        hc_scratch pair_off, keep, is_long, long_idx, sel_idx, counts, status, temp;
        std::vector<hc_scratch> pool;
        std::vector<uint8_t> pool_busy;  // per block of `pool`, during a call: handed out and not given back yet
        hc_scratch edges, next_edges, text, next_text, lines, next_lines;
        uint64_t n_seg[4] = {0, 0, 0, 0}, n_text = 0, n_lines = 0;
        double ms_section[4] = {0, 0, 0, 0};  // hc_fno1_section_ms: the last call's event pairs
        bool valid = false;
        void drop() { valid = false, n_text = n_lines = 0, n_seg[0] = n_seg[1] = n_seg[2] = n_seg[3] = 0; }
    } fno1;
    // hc_br_* (hc_api_br.cpp): the original reads (orig_bases, orig_off: n_orig + 1 offsets) until replaced or hc_reset; the call's vertex
    // tables; grow-only work blocks, each carved into the arrays of hc_br.h: Work by the phase that sizes it (work_v: per vertex, edge and
    // record; work_b: per branch, neighbour and pair; work_d: per diff slot in use; work_e: per item key); the prims' workspace; and the
    // tables (t_*), `counts` of them, valid until the graph, the store or the dict's store is replaced (drop())
    struct Br {
        hc_scratch orig_bases, orig_off;
        uint64_t n_orig = 0;
        bool orig_valid = false;
        hc_scratch vread, vfwd, work_v, work_b, work_d, work_e, temp, counters;
        hc_scratch t_branches, t_nb, t_diff, t_ev_edge, t_ev_off, t_ev_ids, t_missing;
        hc_br_counts counts{};
        bool valid = false;
        // hc_br_reduce: what of hc_br_evidence's work it reads (the slots' records, the kept slots; valid with the tables and while the
        // graph has not been edited since), its own carved block and page-locked staging, and its tables for hc_br_reduce_fetch (host)
        const uint32_t *sl_rec = nullptr, *nb_sel = nullptr;
        uint64_t graph_edits = 0, settings_orc = 0;
        hc_scratch red_work, red_pin = hc_scratch(hipHostMallocDefault);
        std::vector<hc_br_component> red_comps;
        std::vector<uint32_t> red_comp_edge, red_comp_unique, red_removed;
        bool red_valid = false;
        void drop() { valid = false, red_valid = false; }
    } br;
};

namespace hc {
namespace trans {
struct Graph;
}
// hc_api_stage.cpp: what every call that rewrites the graph does first and last (hc_api_label.cpp) — the *_next buffers and the views of
// both graphs; the trade of the buffers once `out` is complete
int graph_clean_prepare(hc_ctx* c, trans::Graph& in, trans::Graph& out);
void graph_clean_commit(hc_ctx* c, const trans::Graph& out);
// hc_api_stage.cpp: the graph edit of hc_br_reduce
int graph_remove_records(hc_ctx* c, const char* who, const uint32_t* d_rec, const uint32_t* d_in_pos, uint64_t n, const hc_edge_rec* d_missing,
                         uint64_t n_missing);
// hc_api_sr.cpp: hc_sr_consensus in parts, for the calls whose layouts are on the device already (hc_api_sr_edge.cpp).
// hc_sr_consensus = its own checks + sr_consensus_begin + sr_consensus_room + the upload of layouts and members + sr_consensus_run.
// `me` prefixes the error texts.  *ret_late (may be NULL): a layout failed late and its ret is no longer the device's.
int sr_consensus_begin(hc_ctx* c, uint64_t* out_off, uint64_t* n_bytes, hc_sr_stats* stats);
int sr_consensus_room(hc_ctx* c, const hc_sr_settings* settings, uint64_t n_layouts, uint64_t n_members);
int sr_consensus_run(hc_ctx* c, const char* me, uint64_t n_layouts, uint64_t n_members, const hc_sr_settings* settings, int32_t* ret, uint32_t* status,
                     uint64_t* out_off, uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats, bool* ret_late);
}  // namespace hc

int hc_ctx_score(hc_ctx* c, uint32_t fmt, const void* d_in, uint64_t n, void* d_out, hipStream_t s, bool reorder,
                 hc_gather_row* rows, unsigned long long* row_count, uint64_t cap, uint64_t base_index,
                 const unsigned long long* n_dev = nullptr, const hc_line_rec* lines_in = nullptr, hc_line_rec* lines_out = nullptr,
                 hc_bucket_ws* bucket = nullptr);  // bucket: the caller's own scratch (launches beside the context's stream), else the context's

// hc_found_to_overlaps with the overlaps file's text left in memory (hc_api_finder.cpp)
int hc_found_to_overlaps_text(hc_ctx* c, uint64_t num_singles, uint64_t num_pairs, std::string& text, uint64_t* n_lines);
