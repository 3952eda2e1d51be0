/*
 * hcsr.h — C ABI of the super-read consensus in libhcedge.so: SRBuilder::consensus and consensus_pos
 * (reference src/SRBuilder.cpp:289-535) for a batch of layouts, on the device against the store of hc_set_reads, and
 * the host mirror of the same contract on plain base / quality arrays.  Plain C, as hcedge.h and hcfno.h.
 * Citations: reference file:line.
 *
 * A LAYOUT is what sort_vertices (src/SRBuilder.cpp:33-285) hands to consensus: total_len and the members in list order
 * (positions ascending, the first is 0).  A MEMBER names a stored sequence instead of carrying strings.
 * Layouts of edge merges: hc_sr_edge_merge; of cliques of any size: hc_sr_clique_merge.
 */
#ifndef HCSR_H_
#define HCSR_H_

#include "hcedge.h"
#include "hcfno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One entry of pos_list / seq_list / qual_list. */
typedef struct hc_sr_member {
    uint32_t read; /* index of the read in the store (hc_set_reads order)                                      */
    int32_t pos;   /* its entry of pos_list                                                                    */
    uint8_t seq;   /* Read::get_seq(0 | 1 | 2): 0 = the sequence of a single-end read, 1 / 2 = mate of a pair   */
    uint8_t rev;   /* 0: get_seq / get_phred; 1: get_rev_comp / get_rev_phred                                  */
    uint8_t pad[2];
} hc_sr_member; /* 12 bytes */

typedef struct hc_sr_layout {
    uint64_t first_member; /* members [first_member, first_member + n_members) of the call's member array */
    uint32_t n_members;
    int32_t total_len;
} hc_sr_layout; /* 16 bytes */

typedef struct hc_sr_settings {
    double min_qual;           /* SRBuilder::minQual, src/SRBuilder.h:89 (0.99 there)                        */
    uint32_t min_clique_size;  /* program_settings.min_clique_size, :426                                    */
    uint32_t error_correction; /* consensus(..., error_correction)                                          */
    uint32_t subreads_needed;  /* consensus(..., subreads_needed): minimumSupport = 2, :422-424             */
    uint32_t n_threads;        /* host threads (the mirror's layouts; the device call's host-finished columns); 0 = 1 */
} hc_sr_settings; /* 24 bytes */

/* Per-layout status: which of the reference's exits a layout took.  cons_seq / cons_qual are empty for all but HC_SR_OK
 * (an HC_SR_OK layout may be empty too: nothing left after the trim). */
enum {
    HC_SR_OK = 0,           /* return trim_pos, :535                                                              */
    HC_SR_NO_SUPPORT = 1,   /* "Not enough support for super-read.", return -1, :441-446                          */
    HC_SR_MEMBER_SHORT = 2, /* a member shorter than its trimmed start, return 0, :490-494                        */
    HC_SR_UNCOVERED = 3,    /* a column no member covers, return 0, :507-510                                      */
    HC_SR_NAN = 4,          /* "p_incorrect NaN", return trim_pos, :367-370, :528-532                             */
    HC_SR_BAD_LAYOUT = 5,   /* refused: no member, member / read index out of range, `seq` that the read does not
                               have, rev > 1, first position not 0, positions not ascending, total_len shorter than
                               a member's end.  Return value 0.  Nothing of the store is read for it.             */
    HC_SR_BAD_SYMBOL = 6    /* a column met a base outside ACGTN or a quality byte outside [33,127] (the
                               reference asserts, :307,340).  Return value 0.                                    */
};

typedef struct hc_sr_stats {
    uint64_t n_columns;      /* consensus positions written                                                         */
    uint64_t n_host_columns; /* of them finished by host threads from the device's four sums (device call only)   */
    double ms_device;        /* device call only: the kernels, by events on the context's stream                  */
    double ms_host_finish;   /* device call only: the host threads' share                                         */
} hc_sr_stats;

/* SRBuilder::consensus (src/SRBuilder.cpp:413-535) with consensus_pos (:296-409) for every layout, on the device.
 * Needs hc_set_reads.  Per layout l: ret[l] = the return value, status[l] = HC_SR_*, and cons_seq / cons_qual hold
 * its bytes at [out_off[l], out_off[l + 1]) — one packed buffer each, out_off has n_layouts + 1 entries.
 * cap = bytes cons_seq and cons_qual each have room for; the sum of the layouts' positive total_len always suffices.
 * *n_bytes = bytes needed; when cap is smaller (or cons_seq / cons_qual are NULL), ret / status / out_off are still
 * filled, nothing is written to the two buffers and HC_ERR_ARG is returned: asking first with cap = 0 and calling again
 * is the count-then-fetch form.  stats may be NULL.
 * Numerics (DESIGN.md "Super-read consensus"): the device adds host-built log10 terms in member order, takes columns
 * of one and two members from a host-built table and decides a deeper column only where the outcome follows from the
 * four sums by comparisons; every other column is finished by host threads with the reference's expressions.  The
 * result is the reference's, byte for byte. */
int hc_sr_consensus(hc_ctx* ctx, const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members, uint64_t n_members,
                    const hc_sr_settings* settings, int32_t* ret, uint32_t* status, uint64_t* out_off, uint8_t* cons_seq,
                    uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats);

/* The same contract on the host, on the arrays hc_set_reads takes (no device, no context): a restatement of
 * :296-535 that walks every layout as the reference does.  What the CPU tests run and what the device is compared with. */
int hc_host_sr_consensus(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                         uint32_t n_reads, const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members,
                         uint64_t n_members, const hc_sr_settings* settings, int32_t* ret, uint32_t* status, uint64_t* out_off,
                         uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats);

/* consensus_pos (:296-409) for ONE column given as strings, by direct evaluation: out[0] = the nucleotide, out[1] = the
 * quality byte.  Returns 1, or 0 where consensus_pos returns 0 (NaN). */
int hc_host_sr_column(const uint8_t* nucleotides, const uint8_t* qualities, uint32_t n, double min_qual, uint8_t* out);

/* The table the device takes columns of one and two members from (built once per call and min_qual on the host by the
 * reference's expressions): entry ((b1 * 5 + b2) * 128 + q1) * 128 + q2 for bases b = 0..4 (A, C, G, T, N) and quality
 * bytes q + 33 of the two members in list order, and, for one member, entry 25 * 128 * 128 + b1 * 128 + q1.
 * (an N member has q = 0 whatever its quality byte: it takes no part).  An entry is the Phred value 0..93, 255 for the 'N' / '$' column, 254 for NaN.  (The nucleotide follows from the exact
 * sums by comparison, :390-393.)  Only q < n_q is filled.  table has HC_SR_TABLE_BYTES bytes. */
#define HC_SR_TABLE_BYTES (25u * 128u * 128u + 5u * 128u)
int hc_host_sr_table(double min_qual, uint32_t n_q, uint8_t* table);

/* Layouts of the simplest real case: merging along an edge between two SINGLE-END reads, as sort_vertices type 's' does
 * for the two vertices of the edge (:33-285): the base is the member with the smaller vertex, the other member's
 * new_pos = pos1 when the base is read 1 of the edge, -pos1 otherwise (:143-148), inserted before the base when
 * new_pos <= 0 (:213-221), positions shifted so that the first is 0 (:247-250), total_len = base length + the two
 * extensions (:236-243).  rev = the vertex is the reverse one (OverlapGraph::getOrientation false).
 * seq_len_by_read[r] = length of single-end read r, paired[r] != 0 marks a paired read (may be NULL: none is).
 * Writes layouts[i] (first_member = 2 i) and members[2 i], members[2 i + 1].  An edge that names a paired read, a read
 * index >= n_reads or read1 == read2 is refused: HC_ERR_BAD_OVERLAP, *first_bad = its index (paired members are not built
 * by THIS call: hc_sr_edge_merge / hc_host_sr_edge_merge_layouts below lay out every combination of read types). */
int hc_host_sr_edge_layouts(const hc_edge_rec* edges, uint64_t n_edges, const uint32_t* seq_len_by_read, const uint8_t* paired,
                            uint32_t n_reads, hc_sr_layout* layouts, hc_sr_member* members, uint64_t* first_bad);

/* ---- edge merges on the device graph: SRBuilder::mergeAlongEdges (src/SRBuilder.cpp:1238-1253) --------------------------
 *
 * mergeAlongEdges takes the cleaned graph, picks the edges to merge (OverlapGraph::getEdgesForMerging,
 * src/GraphAlgos.cpp:112-148) and hands every picked pair of vertices, as a clique of two, to constructSuperread
 * (src/SRBuilder.cpp:654-698), which lays it out with sort_vertices (:33-285) and calls consensus.  The calls of this section
 * do that on the graph the context holds (hc_graph_resolve / hc_graph_load and the cleaning calls), for every combination of
 * single-end and paired reads.
 * Cliques of more than two vertices and filter_subreads (:597-651): hc_sr_clique_merge, the next section.  Clique enumeration
 * (quick-cliques on graph.txt): hc_graph_cliques (include/hcedge.h), on the same graph.  (The `visited` marks and the trivial super-reads of :1260-1373: hc_sr_merge_next; the original-index maps (:750-806) and
 * subreads.txt: hc_sr_originals_next, on the subread infos this call returns.) */

typedef struct hc_merge_pairs_stats {
    double ms_kernel; /* device call only: the target-column kernel, by events on the context's stream */
    double ms_copy;   /* device call only: the copy of the targets and out_off to the host             */
    double ms_walk;   /* the host's walk                                                                */
} hc_merge_pairs_stats; /* 24 bytes */

/* OverlapGraph::getEdgesForMerging (src/GraphAlgos.cpp:112-148) on the context's graph: the sequential greedy matching over the
 * records in (source vertex, list position) order — a vertex that is not marked yet takes its first record whose target is
 * not marked either, and both are marked.  pairs[2 i], pairs[2 i + 1] = (v, w) of the i-th pair taken, in the order taken
 * (the order of process_cliques' input).  cap = pairs the array has room for (n_vertices / 2 always suffices); *n_pairs is
 * always filled; with cap too small (or pairs NULL) nothing is written and HC_ERR_ARG is returned (count, then fetch).
 * The device writes the target column of its out-records as packed 32-bit ids in list order; that array and out_off come
 * back (12 bytes per edge less than the records) and the host walks them: the walk's dependency chain is as long as a path
 * whose ids ascend along it, which is what a cleaned graph looks like.  A graph with tied lists (hc_graph_counts) is
 * refused as by the cleaning calls: HC_ERR_STATE.  stats may be NULL. */
int hc_graph_merge_pairs(hc_ctx* ctx, uint32_t* pairs, uint64_t cap, uint64_t* n_pairs, hc_merge_pairs_stats* stats);

/* The same walk on a caller's records (hc_graph_fetch's edges / out_off; only v2 is read).  A target >= n_vertices:
 * HC_ERR_BAD_OVERLAP. */
int hc_host_graph_merge_pairs(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, uint32_t* pairs, uint64_t cap,
                              uint64_t* n_pairs);

/* Per-pair status of an edge merge: which of the reference's exits the pair took.  Anything but OK: the pair owns no layout. */
enum {
    HC_SR_EDGE_OK = 0,
    HC_SR_EDGE_NO_EDGE = 1,        /* neither base -> node nor node -> base: "Edge not found. Exiting.", src/OverlapGraph.cpp:280   */
    HC_SR_EDGE_BAD_VERTEX = 2,     /* refused: a vertex id >= n_vertices, v == w, or a read index (vertex_read's or the record's)
                                      beyond the store                                                                             */
    HC_SR_EDGE_READ_MISMATCH = 3,  /* neither read of the record is the base's read (assert, src/SRBuilder.cpp:108); or a paired
                                      layout whose record names a single-end read for the other vertex (assert, src/Read.h:145-149) */
    HC_SR_EDGE_PAIRED_NEG_POS = 4, /* a paired member's mate-2 position is negative (assert, :227)                                  */
    HC_SR_EDGE_BAD_GEOMETRY = 5    /* the asserts of :246, :259, :264, :281, or a position / total_len beyond int                   */
};

/* SubreadInfo (src/Types.h:77-82) in the order calcSubreadInfo's caller reads it. */
typedef struct hc_sr_subread_info {
    int32_t index1, startpos1, index2, startpos2;
} hc_sr_subread_info; /* 16 bytes */

/* constructSuperread (src/SRBuilder.cpp:654-698: order, type, base), sort_vertices (:33-285), consensus (:413-535) and
 * calcSubreadInfo (:536-595) for every pair (v, w) = (pairs[2 i], pairs[2 i + 1]) of vertices of the context's graph.
 * Needs hc_set_reads and a graph without tied lists (HC_ERR_STATE otherwise); min_clique_size == 0 is refused with
 * HC_ERR_ARG: the reference then sends a two-vertex clique through filter_subreads (:721), which this call does not build.
 * vertex_read[x] = store index of OverlapGraph::vertex_to_read[x]; vertex_fwd[x] = OverlapGraph::getOrientation(x)
 * (src/OverlapGraph.cpp:83-86); n_vertices must be the graph's.
 * The two vertices are sorted (:658).  Both reads paired: type 'p', TWO layouts ('l', then 'r'), base = the smaller vertex.
 * Otherwise type 's', ONE layout, base = the first single-end read in sorted order (:672-679).  The record is
 * getEdgeInfo(base, node) (src/OverlapGraph.cpp:263-282): the FIRST base -> node of adj_out[base] in list order, else the first
 * node -> base of adj_out[node]; the record's read ids, not its vertices, say whether the base is read 1 (:101-110).
 * Members (:47-76, :114-188): the base takes seq 1 forward / seq 2 reverse-complemented ('l'), seq 2 / seq 1 ('r'), seq 0
 * ('s'); the other vertex likewise by its own orientation, both mates (mate 1, then mate 2) for a paired read in an 's'
 * layout.  new_pos = +-pos1 by whether the base is read 1 ('s', 'l', mate 1); pos2 for mate 2, and for 'r' pos2 when (base is
 * read 1 and ord == '1') or (base is read 2 and ord == '2'), else -pos2.  Every insertion goes in front of the first entry
 * whose position is not smaller (:198-222): the order is (position ascending, insertion number descending).  total_len:
 * :225-244; the shift by -min: :247-252.
 * Outputs.  pair_status[i] = HC_SR_EDGE_*; the layouts of pair i are [first_layout[i], first_layout[i + 1]) (n_pairs + 1
 * entries; n_layouts = first_layout[n_pairs]); layouts (room for 2 n_pairs) and members (room for 6 n_pairs) are packed in pair
 * order, as hc_sr_consensus takes them.  ret / status / out_off (room for 2 n_pairs, 2 n_pairs and 2 n_pairs + 1) / cons_seq /
 * cons_qual / cap / *n_bytes / stats: hc_sr_consensus' outputs for those layouts, by the same code from the device arrays on
 * (with hc_sr_keep_device on, the bytes stay for hc_sr_set_next_reads exactly as after hc_sr_consensus); cap too small:
 * HC_ERR_ARG with everything but the bytes filled.  subreads[2 i], subreads[2 i + 1] = calcSubreadInfo's entries of the
 * smaller and the larger vertex of pair i, with trim_pos1 = ret of the pair's first layout and trim_pos2 = ret of its 'r'
 * layout or -1; a dummy is -1 (:569-570); a paired member of an 's' layout is listed twice, its first entry in list order
 * gives index1 / startpos1 and its second index2 / startpos2; a pair without layouts has all four -1. */
int hc_sr_edge_merge(hc_ctx* ctx, const uint32_t* pairs, uint64_t n_pairs, const uint32_t* vertex_read, const uint8_t* vertex_fwd,
                     uint64_t n_vertices, const hc_sr_settings* settings, uint32_t* pair_status, uint64_t* first_layout,
                     hc_sr_layout* layouts, hc_sr_member* members, hc_sr_subread_info* subreads, int32_t* ret, uint32_t* status,
                     uint64_t* out_off, uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_stats* stats);

/* The layouts and subread infos of hc_sr_edge_merge on the host (no device, no context): a graph as hc_graph_fetch returns it
 * (edges, out_off) and the read table as hc_set_reads takes it (seq_off, read_first_seq); it walks the lists and inserts
 * into a position list as the reference does.  ret (per layout, what a consensus call returned for them) is an INPUT of the
 * subread infos; with ret NULL subreads is not written — call once for the layouts, run the consensus, call again. */
int hc_host_sr_edge_merge_layouts(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, const uint64_t* seq_off,
                                  const uint32_t* read_first_seq, uint32_t n_reads, const uint32_t* pairs, uint64_t n_pairs,
                                  const uint32_t* vertex_read, const uint8_t* vertex_fwd, const hc_sr_settings* settings,
                                  uint32_t* pair_status, uint64_t* first_layout, hc_sr_layout* layouts, hc_sr_member* members,
                                  const int32_t* ret, hc_sr_subread_info* subreads);

/* ---- cliques of any size on the device graph: SRBuilder::cliquesToSuperreads -> process_cliques -> constructSuperread ----------
 *
 * constructSuperread (src/SRBuilder.cpp:654-748) for a clique of any number of vertices: the sort of the clique (:658), the type
 * and base choice (:669-679), sort_vertices (:33-285) with getEdgeInfo(base, node) for every member (src/OverlapGraph.cpp:263-282),
 * filter_subreads / sortVerticesByEndpos (:597-651) where the clique is larger than 3 * min_clique_size (:721), consensus
 * (:413-535) and calcSubreadInfo (:536-595).
 * Left to the caller: reading cliques.txt, remove_multi_occ and the minCliqueSize gate (:1056-1084; remove_multi_occ is a serial
 * greedy pass over a text file: hc_host_sr_clique_select).  The cliques themselves: hc_graph_cliques (include/hcedge.h), whose
 * hc_graph_cliques_fetch arrays are this call's clique_off / clique_nodes.  (The original-index maps (:750-806) and
 * subreads.txt: hc_sr_originals_next, on the subread infos this call returns.)
 * The marks, the trivials, the next store and the FNO tables from these outputs: hc_sr_clique_next. */

/* Per-clique status: the HC_SR_EDGE_* values and two more.  Where several members of a clique fail, the status is that of the first
 * failing vertex in the loop's order (ascending vertex, :658, :87) and within a vertex the reference's order of checks; the asserts
 * behind the loop (:246-281, HC_SR_EDGE_BAD_GEOMETRY) count only if the loop passed.  The range checks run before the loop: a clique
 * with a vertex >= n_vertices or a vertex_read beyond the store is HC_SR_EDGE_BAD_VERTEX and reads nothing further. */
enum {
    HC_SR_CLIQUE_TOO_SMALL = 6,       /* fewer than two vertices (assert, :656)                                                        */
    HC_SR_CLIQUE_REPEATED_VERTEX = 7  /* a vertex listed twice: a stated tightening, as v == w is for pairs (a clique of exactly two
                                         equal vertices reports HC_SR_EDGE_BAD_VERTEX, as hc_sr_edge_merge does)                       */
};

/* What filter_subreads did to a layout.  sortVerticesByEndpos ends in an unstable std::sort (:640); the selection walks the endpos
 * groups from the largest down, and only a group that is cut depends on the order among its ties (host/SrCliqueFilter.h). */
enum {
    HC_SR_FILTER_NONE = 0,   /* clique.size() <= 3 * min_clique_size: every member is used                                             */
    HC_SR_FILTER_GROUPS = 1, /* only whole groups of equal endpos were taken: the order among ties cannot matter                       */
    HC_SR_FILTER_STABLE = 2, /* a group was cut in a layout of at most 16 entries: libstdc++'s std::sort is one insertion sort there,
                                which is stable, so the cut takes the group's entries from the back of the list order                  */
    HC_SR_FILTER_HOST = 3    /* a group was cut in a longer layout: decided by std::sort itself, on the host                           */
};

typedef struct hc_sr_clique_stats {
    hc_sr_stats sr;              /* the consensus' share, as hc_sr_consensus reports it                                                 */
    uint64_t n_filtered_layouts; /* layouts that went through filter_subreads                                                           */
    uint64_t n_host_filters;     /* of them HC_SR_FILTER_HOST (device call: decided by host threads)                                    */
    double ms_layout;            /* device call only: the layout, filter and subread kernels, by events on the context's stream         */
    double ms_host_filter;       /* device call only: fetching, deciding and uploading the host-decided filters                         */
} hc_sr_clique_stats; /* 64 bytes */

/* constructSuperread for every clique i = clique_nodes[clique_off[i] .. clique_off[i + 1]) (process_cliques' clique_vec, :980, as a
 * CSR of vertex ids, in any order inside a clique) on the context's graph.  N = clique_off[n_cliques] entries in all.
 * Needs hc_set_reads and a graph without tied lists (HC_ERR_STATE otherwise).  HC_ERR_ARG: min_clique_size == 0 (with num == 0 the
 * filter may drop the first list entry, a layout hc_sr_consensus refuses); n_vertices is not the graph's; descending clique_off;
 * N >= 2^31 or 2^32 records or more.  vertex_read / vertex_fwd: as hc_sr_edge_merge takes them.
 * A clique of two gives exactly what hc_sr_edge_merge gives for the same pair.
 * Outputs, packed in clique order: clique_status[i]; first_layout (n_cliques + 1: one layout for type 's', two for 'p', 'l' then 'r');
 * layouts (room for 2 n_cliques) and members / member_vertex / member_used (room for 2 N each): the FULL lists sort_vertices returned,
 * as hc_sr_consensus takes them — member_vertex = sorted_vertices1 / sorted_vertices2, which set_sorted_clique keeps (:853-864);
 * member_used = 1 where the member was handed to consensus (all unless clique.size() > 3 * min_clique_size, else filter_subreads' choice
 * for num = 2 * min_clique_size); layout_filter (room for 2 n_cliques; may be NULL): HC_SR_FILTER_*.
 * ret / status / out_off (2 n_cliques, 2 n_cliques, 2 n_cliques + 1) / cons_seq / cons_qual / cap / *n_bytes: hc_sr_consensus' outputs
 * for the USED members of each layout with the layout's full total_len (:725-741), by the same code (with hc_sr_keep_device on, the bytes
 * stay on the device exactly as after hc_sr_consensus); cap too small: HC_ERR_ARG with everything but the bytes filled.
 * subreads (room for N): calcSubreadInfo on the FULL lists with trim_pos1 / trim_pos2 = the ret of the layouts (:748), one entry per
 * clique vertex in ASCENDING VERTEX order at clique_off[i] (deterministic, not the unordered_map's order): a vertex's first entry in
 * list 1 gives index1 / startpos1, its second entry in list 1 (a paired read in an 's' layout) or its entry in list 2 ('p') index2 /
 * startpos2; a dummy is -1; a clique without layouts has all four -1.  stats may be NULL. */
int hc_sr_clique_merge(hc_ctx* ctx, const uint64_t* clique_off, const uint32_t* clique_nodes, uint64_t n_cliques, const uint32_t* vertex_read,
                       const uint8_t* vertex_fwd, uint64_t n_vertices, const hc_sr_settings* settings, uint32_t* clique_status,
                       uint64_t* first_layout, hc_sr_layout* layouts, hc_sr_member* members, uint32_t* member_vertex, uint8_t* member_used,
                       uint8_t* layout_filter, hc_sr_subread_info* subreads, int32_t* ret, uint32_t* status, uint64_t* out_off,
                       uint8_t* cons_seq, uint8_t* cons_qual, uint64_t cap, uint64_t* n_bytes, hc_sr_clique_stats* stats);

/* A test switch of the context, off by default: while on, hc_sr_clique_merge sends EVERY filtered layout to the host's filter.  The
 * outputs must not change (layout_filter still reports the classification). */
int hc_sr_clique_filter_on_host(hc_ctx* ctx, int on);

/* The layouts, the filter's choice and the subread infos of hc_sr_clique_merge on the host (no device, no context): a graph as
 * hc_graph_fetch returns it and the read table as hc_set_reads takes it.  It walks the reference's loops as written: std::list
 * insertions, a std::set of selected vertices and std::sort with the reference's comparator on a vector in list order.  ret (per
 * layout, what a consensus call returned for the USED members) is an INPUT of the subread infos; with ret NULL subreads is not written.
 * stats (may be NULL): n_filtered_layouts and n_host_filters. */
int hc_host_sr_clique_merge_layouts(const hc_edge_rec* edges, const uint64_t* out_off, uint64_t n_vertices, const uint64_t* seq_off,
                                    const uint32_t* read_first_seq, uint32_t n_reads, const uint64_t* clique_off, const uint32_t* clique_nodes,
                                    uint64_t n_cliques, const uint32_t* vertex_read, const uint8_t* vertex_fwd, const hc_sr_settings* settings,
                                    uint32_t* clique_status, uint64_t* first_layout, hc_sr_layout* layouts, hc_sr_member* members,
                                    uint32_t* member_vertex, uint8_t* member_used, uint8_t* layout_filter, const int32_t* ret,
                                    hc_sr_subread_info* subreads, hc_sr_clique_stats* stats);

/* filter_subreads' selection (:597-622) for ONE layout given as (vertex, endpos) per entry in list order: used[k] = 1 where entry k's
 * vertex is selected; *filter = HC_SR_FILTER_GROUPS / _STABLE / _HOST by the shared group rule.  tie_order chooses how ties of
 * sortVerticesByEndpos are ordered: 0 = std::sort with the reference's comparator (the reference), 1 = list order inside every group
 * (a stable sort), 2 = reversed list order inside every group.  HC_ERR_ARG: n == 0, num > the layout's distinct vertices (the
 * reference asserts, :619), or the base is no entry. */
int hc_host_sr_clique_filter(const uint32_t* vertex, const int32_t* endpos, uint32_t n, uint32_t num, uint32_t base_vertex, int tie_order,
                             uint8_t* used, uint32_t* filter);

/* ---- self-overlapping paired super-reads: SRBuilder::merge_self_overlap (src/SRBuilder.cpp:872-955) --------------------
 *
 * process_cliques (src/SRBuilder.cpp:958-1029) hands every paired super-read with two non-empty mates to merge_self_overlap,
 * which slides mate 2 along mate 1 from the smallest allowed overlap on (:879-888), scores every offset with
 * EdgeCalculator::overlap_score (src/EdgeCalculator.cpp:67-139) and replaces the pair, at the first offset that scores above
 * min_score, by the two-member consensus of the mates (:890-903) as one single-end super-read.
 *
 * A PAIR names its two mates inside one packed base buffer and one packed quality buffer — what hc_sr_consensus writes
 * (cons_seq, cons_qual, out_off), so that a caller passes those buffers on unchanged. */
typedef struct hc_sr_pair {
    uint64_t off1, off2; /* first byte of mate 1 / mate 2 in seq and qual */
    uint32_t len1, len2;
} hc_sr_pair; /* 24 bytes */

typedef struct hc_sr_self_settings {
    double min_score;     /* 0.99, src/SRBuilder.cpp:874                                                          */
    double min_qual;      /* SRBuilder::minQual for the consensus of the merged read, src/SRBuilder.h:89          */
    uint32_t min_overlap; /* 15, src/SRBuilder.cpp:873                                                            */
    uint32_t n_threads;   /* host threads (the mirror's pairs; the device call's checks and host-decided pairs); 0 = 1 */
} hc_sr_self_settings; /* 24 bytes */

/* Per-pair status. */
enum {
    HC_SR_SELF_NONE = 0,      /* no offset scored above min_score: the pair stays as it is, return superread, :954       */
    HC_SR_SELF_MERGED = 1,    /* merged at overlap_pos, :890-950                                                         */
    HC_SR_SELF_BAD_PAIR = 2,  /* refused: len1 == 0, len2 == 0 (the asserts of src/EdgeCalculator.cpp:70-73), a mate that
                                 does not lie inside n_bytes, or len1 + len2 > INT32_MAX (overlap_pos is an int32_t and
                                 the merged read has up to len1 + len2 - 1 columns).  Nothing of the buffers is read for
                                 it.                                                                                    */
    HC_SR_SELF_BAD_SYMBOL = 3 /* a base outside ACGTN or a quality byte outside [33,126] ANYWHERE in either mate.  The
                                 reference asserts on such a symbol when an offset touches it
                                 (src/EdgeCalculator.cpp:29-30,61); checking the whole pair before the scan is a stated
                                 tightening: a pair whose bad symbol no tried offset would have reached is refused too. */
};

typedef struct hc_sr_self_stats {
    uint64_t n_merged;     /* pairs with HC_SR_SELF_MERGED                                                              */
    uint64_t n_host_pairs; /* device call only: pairs whose deciding offset fell into the guard band of min_score (or
                              whose consensus table holds a NaN entry) and that host threads finished                  */
    uint64_t n_offsets;    /* offsets the batch holds in all, sum of max(len1 - min_overlap, 0) over the valid pairs:
                              what a batch that merges nothing scans                                                   */
    double ms_device;      /* device call only: the kernels, by events on the context's stream                         */
    double ms_host;        /* device call only: the host threads' share (checks, table, host-decided pairs)            */
} hc_sr_self_stats;

/* merge_self_overlap (src/SRBuilder.cpp:872-955) for every pair, on the device.  Needs no hc_set_reads; --mismatch and
 * --min_read_len are those of the context's hc_settings, as EdgeCalculator takes them from program_settings
 * (src/EdgeCalculator.cpp:49,82).
 * The scan of pair i (:879-888): the offsets p = len1 - min_overlap, len1 - min_overlap - 1, ..., 1 in that order (none
 * when len1 <= min_overlap; p = 0 is never tried), each scored over L = min(len1 - p, len2) positions: 0 when a mate is
 * shorter than min_read_len, when a position's probability lies below --mismatch or when every position holds an N, else
 * exp((1.0 / n) * sum of log p_i) with the terms added in position order.  The first p with score > min_score is taken.
 * The merge (:890-903): consensus() of {mate 1 at 0, mate 2 at p}, total_len = len2 + p, no error correction — column c
 * holds mate 1 when c < len1 and mate 2 when c >= p; with len2 + p < len1 the output stops at total_len (a layout
 * hc_sr_consensus refuses and consensus() as called here does not).  Where consensus() comes back empty (the NaN exit of
 * consensus_pos) the scan goes on with the next offset (:904).
 * Outputs per pair: overlap_pos[i] = p or -1; score[i] = overlap_score's value at p (host exp) or 0; status[i] = HC_SR_SELF_*;
 * the merged bytes of pair i at [out_off[i], out_off[i + 1]) of merged_seq / merged_qual (out_off has n_pairs + 1 entries; an
 * unmerged pair owns no bytes).  cap / *n_out: as hc_sr_consensus' cap / *n_bytes, cap = 0 with NULL buffers is the count of
 * count-then-fetch (HC_ERR_ARG, everything but the bytes filled).  stats may be NULL.
 * Left to the caller: index2 += p in the subread map and in the original indexes and the re-sort of the clique by
 * index (:911-949), and Read::test_N_rate (src/Read.h:214-234).  (The mates on the device already: hc_sr_merge_self_overlaps_kept.)
 * Numerics (DESIGN.md "Self-overlap merge"): the device adds host-built log p terms, one lane per offset, in position order;
 * score > min_score is decided on x = (1.0 / n) * sum against the x-space image of min_score, an offset inside the guard band
 * goes to the host's libm; the merged bytes come from hc_host_sr_table.  The result is the reference's, byte for byte. */
int hc_sr_merge_self_overlaps(hc_ctx* ctx, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes, const hc_sr_pair* pairs,
                              uint64_t n_pairs, const hc_sr_self_settings* settings, int32_t* overlap_pos, double* score,
                              uint32_t* status, uint64_t* out_off, uint8_t* merged_seq, uint8_t* merged_qual, uint64_t cap,
                              uint64_t* n_out, hc_sr_self_stats* stats);

/* ---- the same merge from the consensus bytes the context keeps ------------------------------------------------------------
 *
 * Between hc_sr_consensus / hc_sr_edge_merge with hc_sr_keep_device on, which leave their bytes on the device, and
 * hc_sr_set_next_reads, which builds the next store from them, sits process_cliques' self-overlap test
 * (src/SRBuilder.cpp:982-996).  The calls below run it without bringing the bytes to the host and back. */

/* merge_self_overlap (src/SRBuilder.cpp:872-955) for every pair, the mates read from the KEPT consensus bytes and the merged
 * reads APPENDED to them.  The contract is hc_sr_merge_self_overlaps' word for word — the offsets tried and their order
 * (:879-888), the early exit at the first offset above min_score, the merge (:890-903, going on at :904 where consensus() comes
 * back empty), the statuses including the stated tightening of HC_SR_SELF_BAD_SYMBOL, the guard band and the host's exp — with
 * two differences: off1 / off2 index the kept bytes as they stand when the call starts, and n_bytes is the kept size.
 * Outputs per pair: overlap_pos / score / status as there.  The merged bytes of pair i are written to the kept buffers at
 * [out_off[i], out_off[i + 1]): ABSOLUTE offsets into the kept bytes, out_off[0] = the kept size on entry, n_pairs + 1 entries.
 * *n_out = bytes appended.  The kept size grows by *n_out on success and is untouched on any error.  A second call appends
 * behind the first, and its pairs may name bytes the first appended; hc_sr_set_next_reads names the merged reads as
 * HC_SR_SRC_CONSENSUS at out_off[i]; the next hc_sr_consensus / hc_sr_edge_merge replaces the kept bytes as it does without
 * this call, the appended region included.
 * HC_ERR_STATE: hc_sr_keep_device is off, or nothing is kept.  n_pairs == 0: HC_OK, out_off[0] = the kept size.
 * The pairs are checked on the device (the range test is the host's own function, and nothing is read for an
 * HC_SR_SELF_BAD_PAIR); stats->ms_host counts only the tables and the host-decided pairs, stats->ms_device the check kernel too.
 * Nothing of the mates or the merged reads crosses the link but the mates of the pairs the host decides.  stats may be NULL.
 * Left to the caller, as with hc_sr_merge_self_overlaps: index2 += p in the subread map and in the original indexes and the
 * re-sort of the clique by index (src/SRBuilder.cpp:911-949), and Read::test_N_rate (src/Read.h:214-234; hc_sr_set_next_reads
 * applies it). */
int hc_sr_merge_self_overlaps_kept(hc_ctx* ctx, const hc_sr_pair* pairs, uint64_t n_pairs, const hc_sr_self_settings* settings,
                                   int32_t* overlap_pos, double* score, uint32_t* status, uint64_t* out_off, uint64_t* n_out,
                                   hc_sr_self_stats* stats);

/* Makes the caller's bytes the kept consensus bytes (n_bytes each; 0 is allowed: kept, and empty), as if the last
 * hc_sr_consensus had written them: for super-reads that come from somewhere other than this context's last consensus call —
 * process_cliques (src/SRBuilder.cpp:958-1029) takes its super-reads from whichever constructSuperread made them.
 * HC_ERR_STATE: hc_sr_keep_device is off.  Left to the caller: that the bytes are super-reads at all; nothing is checked here,
 * the calls that read them check what they read. */
int hc_sr_kept_load(hc_ctx* ctx, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes);

/* Copies [off, off + n) of the kept consensus bytes out — the merged reads of hc_sr_merge_self_overlaps_kept for whoever
 * writes them as text (src/SRBuilder.cpp:1416-1556), off the critical path.  *n_kept = the kept size, always filled (0 when
 * nothing is kept: HC_ERR_STATE).  A range that does not lie inside the kept bytes: HC_ERR_ARG, nothing copied.  n = 0 asks for
 * the size alone.  Left to the caller: which bytes of them are whose read (the FASTQ text of a store: hc_sr_fastq_write_text). */
int hc_sr_kept_fetch(hc_ctx* ctx, uint64_t off, uint64_t n, uint8_t* seq, uint8_t* qual, uint64_t* n_kept);

/* The same contract on the host (no device, no context): overlap_score (src/EdgeCalculator.cpp:26-139) offset by offset and
 * consensus_pos column by column, as the reference walks them, on settings->n_threads threads.  Of hc_settings only
 * mismatch and min_read_len are read. */
int hc_host_sr_merge_self_overlaps(const hc_settings* ec_settings, const uint8_t* seq, const uint8_t* qual, uint64_t n_bytes,
                                   const hc_sr_pair* pairs, uint64_t n_pairs, const hc_sr_self_settings* settings,
                                   int32_t* overlap_pos, double* score, uint32_t* status, uint64_t* out_off, uint8_t* merged_seq,
                                   uint8_t* merged_qual, uint64_t cap, uint64_t* n_out, hc_sr_self_stats* stats);

/* ---- the next iteration's read store from super-reads, without leaving the device ---------------------------------------
 *
 * Between one SAVAGE / POLYTE iteration and the next the reference filters the super-reads (process_cliques,
 * src/SRBuilder.cpp:983,986-996,999-1001; Read::get_len / test_N_rate, src/Read.h:203-234), numbers the survivors and adds
 * the trivial super-reads (src/SRBuilder.cpp:1141-1233,1278-1380: single-end super-reads from id 0, the trivial ones in
 * vertex order, the paired ones last), writes them as FASTQ (:1416-1556: decimal ids, the sequences as stored) and reads the
 * files again.  hc_sr_set_next_reads does the filtering, the numbering and the copying on the device and replaces the
 * context's read store by the result.
 * Left to the caller: the files themselves.  (The FASTQ text of the new store: hc_sr_fastq_write_text, the last section.  The
 * original-index maps and subreads.txt: hc_sr_originals_next / hc_sr_originals_write_text, from the subread infos of hc_sr_edge_merge /
 * hc_sr_clique_merge.)  With hc_sr_set_next_reads the caller also lists the entries: it omits the vertices of :1298-1311 and re-sorts a
 * clique that merge_self_overlap merged (:911-949) itself; hc_sr_merge_next below builds the list, the marks, the tips and the
 * shifted cliques from an edge merge's outputs.  (The self-overlap test between the consensus call and this one runs on the kept
 * bytes: hc_sr_merge_self_overlaps_kept.) */

/* Off by default: every other call then behaves and allocates as it does without this section.  While it is on, hc_set_reads
 * keeps its device copies of the raw base, quality and offset arrays (trivial super-reads are copied from them: the encoded
 * store cannot serve, its wide encodings drop the quality byte of an N) and hc_sr_consensus leaves its packed cons_seq /
 * cons_qual bytes on the device in their final form (the columns host threads finish are written back by one scatter launch;
 * the bytes returned to the host are the same).  Turning it off releases what was kept. */
int hc_sr_keep_device(hc_ctx* ctx, int on);

enum {
    HC_SR_NEXT_SINGLE = 0,        /* a single-end super-read: mate 1 only                                                    */
    HC_SR_NEXT_PAIRED = 1,        /* a paired super-read: mate 1 and mate 2                                                  */
    HC_SR_NEXT_TRIVIAL = 2,       /* a trivial super-read: single-end read `read` of the current store                       */
    HC_SR_NEXT_TRIVIAL_PAIRED = 3 /* the same for a paired read (the writers send the two to different files, :1461-1500)    */
};
enum {
    HC_SR_SRC_CONSENSUS = 0, /* the kept cons_seq / cons_qual of the last hc_sr_consensus (the mirror: the arrays passed)   */
    HC_SR_SRC_BYTES = 1      /* extra_seq / extra_qual of this call: hc_sr_merge_self_overlaps' merged reads, or anything
                                else the caller holds on the host                                                          */
};

/* One candidate read of the next iteration. */
typedef struct hc_sr_next_entry {
    uint64_t off1, off2; /* a super-read: first byte of mate 1 / mate 2 in its source                                    */
    uint32_t len1, len2; /* a super-read: their lengths (len2 is not read for HC_SR_NEXT_SINGLE)                          */
    uint32_t read;       /* a trivial: index of the read in the current store                                            */
    uint8_t kind;        /* HC_SR_NEXT_*                                                                                 */
    uint8_t src1, src2;  /* a super-read: HC_SR_SRC_* of mate 1 / mate 2                                                  */
    uint8_t rev;         /* a trivial: 1 = the reverse vertex, taken as rev_comp(0) or (rev_comp(2), rev_comp(1)) with the
                            reversed Phred strings (:1342,1355)                                                         */
} hc_sr_next_entry; /* 32 bytes */

typedef struct hc_sr_next_settings {
    uint32_t keep_singletons; /* program_settings.keep_singletons, :1286 */
    uint32_t reserved;
} hc_sr_next_settings; /* 8 bytes */

/* Per-entry status.  The tests run in this order. */
enum {
    HC_SR_NEXT_KEPT = 0,
    HC_SR_NEXT_DROPPED_EMPTY = 1,  /* a super-read with an empty mate: get_seq(0) == "" (:999), get_seq(1) or get_seq(2) == ""
                                      (:983: the pair is dropped whole)                                                   */
    HC_SR_NEXT_DROPPED_N_RATE = 2, /* test_N_rate is false: not (double)N_count < 0.05 * (double)len, over the
                                      concatenation of the mates for a pair (src/Read.h:214-234)                          */
    HC_SR_NEXT_DROPPED_SHORT = 3,  /* a trivial with get_len() < keep_singletons, len1 + len2 for a pair (:1286; tested
                                      before the N rate, :1292)                                                           */
    HC_SR_NEXT_BAD_ENTRY = 4       /* refused: kind > 3, src > 1, rev > 1, a range that does not lie inside its source, a
                                      mate of 2^28 bytes or more (hc_set_reads refuses such a sequence), a read index >=
                                      the store's reads, HC_SR_NEXT_TRIVIAL on a paired read or HC_SR_NEXT_TRIVIAL_PAIRED
                                      on a single-end one.  Nothing is read for it.                                       */
};

typedef struct hc_sr_next_counts {
    uint64_t n_kept, n_dropped_empty, n_dropped_n_rate, n_dropped_short, n_bad;
    uint64_t n_seq;   /* sequences of the new store  */
    uint64_t n_bytes; /* bases of the new store      */
    double ms_device; /* device call only: the kernels of this section, by events on the context's stream */
    double ms_plan;   /* device call only: the host's planning between them and the encoder              */
} hc_sr_next_counts; /* 72 bytes */

/* hc_sr_set_next_reads: HC_OK is 0; an empty result is no error of the arguments and has a status of its own. */
#define HC_SR_NEXT_EMPTY 1

/* Needs hc_sr_keep_device(ctx, 1) before the hc_set_reads that loaded the current store (HC_ERR_STATE otherwise).
 * The entries are taken in the order given — the caller lists them as the writers do: singles, trivials, pairs — and
 * new_id[i] = the rank of entry i among the kept ones (the read's index in the new store and its decimal FASTQ id), or -1;
 * status[i] = HC_SR_NEXT_*.  extra_seq / extra_qual (n_extra bytes each, may be NULL with n_extra = 0) are uploaded by the call.
 * A reverse trivial is written back to front with build_rev_comp's mapping (Types.h:109-129: A<->T, C<->G, N->N; any other byte,
 * on which the reference exits, is copied as it is and the new store flags the sequence as hc_set_reads does).
 * The survivors' raw bytes are gathered into new raw arrays on the device, and the context's store is replaced from them
 * exactly as hc_set_reads would replace it from the same arrays on the host: the same quality map, encoding, slot alignment,
 * `regular` flag, locality order and tables, and the same dependent state is invalidated.  The new raw arrays become the kept
 * ones; the kept consensus bytes stay as they are.
 * When nothing is kept: HC_SR_NEXT_EMPTY, new_id / status / counts filled, the old store in place.
 * counts may be NULL. */
int hc_sr_set_next_reads(hc_ctx* ctx, const hc_sr_next_entry* entries, uint64_t n, const uint8_t* extra_seq, const uint8_t* extra_qual,
                         uint64_t n_extra, const hc_sr_next_settings* settings, int32_t* new_id, uint32_t* status,
                         hc_sr_next_counts* counts);

/* The kept raw arrays — what hc_set_reads or hc_sr_set_next_reads last loaded while keeping was on — in the form
 * hc_set_reads takes: for the writer of singles.fastq / paired*.fastq, once, off the critical path.
 * *n_bytes / *n_seq / *n_reads are always filled.  cap_bytes = room of bases and quals each, cap_seq = entries seq_off has
 * room for beyond its first (n_seq + 1 are written) and read_first_seq likewise (n_reads + 1 <= n_seq + 1 are written);
 * where either is too small or a buffer is NULL nothing is copied and HC_ERR_ARG is returned (count, then fetch). */
int hc_sr_next_reads_fetch(hc_ctx* ctx, uint8_t* bases, uint8_t* quals, uint64_t cap_bytes, uint64_t* seq_off, uint32_t* read_first_seq,
                           uint64_t cap_seq, uint64_t* n_bytes, uint64_t* n_seq, uint64_t* n_reads);

/* The same contract on the host (no device, no context): the current store as hc_set_reads takes it, the consensus bytes
 * (n_cons each), the entries — and the four arrays one would pass to hc_set_reads next.  out_seq_off needs room for
 * 2 n + 1 entries and out_read_first_seq for n + 1; cap / *n_bytes as above (too small or NULL: HC_ERR_ARG, everything but
 * the bytes filled).  An empty result returns HC_SR_NEXT_EMPTY. */
int hc_host_sr_next_reads(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                          uint32_t n_reads, const uint8_t* cons_seq, const uint8_t* cons_qual, uint64_t n_cons,
                          const hc_sr_next_entry* entries, uint64_t n, const uint8_t* extra_seq, const uint8_t* extra_qual,
                          uint64_t n_extra, const hc_sr_next_settings* settings, int32_t* new_id, uint32_t* status,
                          hc_sr_next_counts* counts, uint8_t* out_bases, uint8_t* out_quals, uint64_t cap, uint64_t* n_bytes,
                          uint64_t* out_seq_off, uint32_t* out_read_first_seq);

/* ---- the rest of mergeAlongEdges in one call: marks, trivials, the next store and the FNO tables --------------------------
 *
 * Between hc_sr_edge_merge and find-next-overlaps SRBuilder::mergeAlongEdges (src/SRBuilder.cpp:1238-1384) judges the super-reads
 * (process_cliques, :981-1001, with merge_self_overlap, :872-955), marks the vertices of the survivors (:1260-1277), walks the
 * unvisited vertices for the trivial super-reads (:1282-1373) and numbers the three groups (:1279-1280, :1370-1371, :1378).
 * hc_sr_merge_next does that on the device from what hc_sr_edge_merge returned: it leaves the next store in the context, as
 * hc_sr_set_next_reads would for the same entries in the same order, and returns the vertex and super-read tables of an
 * hc_fno1_input (hcfno.h) ready to use.
 * The semantics are the reference's with N_THREADS = 1: with more threads process_cliques concatenates per-thread blocks in
 * arrival order (:1004-1011), which is not deterministic; one thread gives pair order.
 * Left to the caller: appending the texts to the files.  The FASTQ text, including removed_tip_sequences.fastq: hc_sr_fastq_write_text,
 * the last section, which takes this call's tips list and vertex_read as they are.  The original-index maps
 * (:750-806, :1312-1369) and subreads.txt: hc_sr_originals_next, below, on this call's outputs.  This call for cliques of more than two vertices is
 * hc_sr_clique_next, below, on hc_sr_clique_merge's outputs. */

typedef struct hc_sr_merge_next_input {
    /* what hc_sr_edge_merge returned, unchanged: host arrays */
    const uint32_t* pairs;              /* (v, w) of pair i = pairs[2 i], pairs[2 i + 1]: process_cliques' clique_vec, :980              */
    uint64_t n_pairs;
    const uint32_t* pair_status;        /* HC_SR_EDGE_*: anything but OK owns no super-read (constructSuperread asserted or exited, :981) */
    const uint64_t* first_layout;       /* n_pairs + 1: one layout = single-end, two = paired (:850-869)                                 */
    const hc_sr_layout* layouts;        /* first_layout[n_pairs] of them: the first one's members give get_sorted_clique (:853, :864)     */
    const hc_sr_member* members;
    uint64_t n_members;                 /* entries of members: at most 6 n_pairs, what hc_sr_edge_merge has room for (HC_ERR_ARG beyond)  */
    const uint32_t* status;             /* HC_SR_* per layout: a layout that is not HC_SR_OK is an empty mate (:983, :999)               */
    const uint64_t* out_off;            /* n_layouts + 1: cons_seq1 / cons_seq2 (:852, :863) among the KEPT consensus bytes              */
    const hc_sr_subread_info* subreads; /* 2 n_pairs: calcSubreadInfo's entries of the smaller and the larger vertex (:536-595)          */
    /* the graph's vertices */
    const uint32_t* vertex_read;        /* OverlapGraph::vertex_to_read as store indices, :1284                                          */
    const uint8_t* vertex_fwd;          /* OverlapGraph::getOrientation, :1331                                                           */
    uint64_t n_vertices;                /* OverlapGraph::getVertexCount, :1261, :1282                                                    */
    const uint8_t* inclusions;          /* OverlapGraph::inclusions, one byte per vertex (hc_graph_fetch), :1298; NULL: none             */
    const uint8_t* tip_reads;           /* Read::is_tip(), :1305: one byte for EVERY read of the current store (hc_graph_fetch_tip_reads
                                           with n_reads = the store's reads); the call reads that many and cannot check it; NULL: none  */
} hc_sr_merge_next_input;

typedef struct hc_sr_merge_next_settings {
    uint32_t keep_singletons;       /* program_settings.keep_singletons, :1286                                              */
    uint32_t ignore_inclusions;     /* program_settings.ignore_inclusions, :1298                                            */
    uint32_t store_tips_separately; /* program_settings.store_tips_separately, :1305                                        */
    uint32_t no_self_overlap;       /* 1: merge_self_overlap (:985) is left out, every paired super-read stays paired       */
    hc_sr_self_settings self;       /* merge_self_overlap's constants (:873-874: min_score 0.99, min_overlap 15) and minQual */
} hc_sr_merge_next_settings; /* 40 bytes */

/* What became of pair i. */
enum {
    HC_SR_MN_NONE = 0,            /* no super-read: pair_status is not HC_SR_EDGE_OK, or the pair's layouts / vertices are refused     */
    HC_SR_MN_DROPPED_EMPTY = 1,   /* an empty mate, :983, :999                                                                         */
    HC_SR_MN_DROPPED_N_RATE = 2,  /* test_N_rate false, :986, :999 (of the merged read for a pair that self-merged)                    */
    HC_SR_MN_SINGLE = 3,          /* singles_this_thread, :1000                                                                        */
    HC_SR_MN_SINGLE_SELF = 4,     /* a paired super-read merge_self_overlap merged, :993-995                                           */
    HC_SR_MN_PAIRED = 5           /* pairs_this_thread, :990-992                                                                       */
};
/* What became of vertex v; the tests of an unvisited vertex run in this order (:1286-1311). */
enum {
    HC_SR_MN_V_MERGED = 0,    /* visited by a surviving super-read, :1264-1275                                                         */
    HC_SR_MN_V_TRIVIAL = 1,   /* a trivial super-read, :1312-1371                                                                      */
    HC_SR_MN_V_SHORT = 2,     /* get_len() < keep_singletons, :1286                                                                    */
    HC_SR_MN_V_N_RATE = 3,    /* test_N_rate false, :1292                                                                              */
    HC_SR_MN_V_INCLUSION = 4, /* ignore_inclusions && inclusions[v], :1298: on the tips list                                           */
    HC_SR_MN_V_TIP = 5,       /* is_tip() && store_tips_separately, :1305: on the tips list                                            */
    HC_SR_MN_V_BAD = 6        /* refused: vertex_read[v] is no read of the store.  Marked visited, no id.                              */
};

typedef struct hc_sr_merge_next_output {
    /* per pair (n_pairs entries each) */
    uint32_t* pair_kind;   /* HC_SR_MN_*                                                                                               */
    int32_t* pair_new_id;  /* Read id of the pair's super-read in the next store (:1280, :1378) or -1                                  */
    int32_t* overlap_pos;  /* merge_self_overlap's overlap_pos (:882) of a pair it merged, else -1                                     */
    double* self_score;    /* overlap_score's value there (:886), else 0                                                               */
    /* per vertex (n_vertices entries each) */
    uint32_t* vertex_state; /* HC_SR_MN_V_*                                                                                            */
    hc_fno_read* nodes;     /* id = nodes_to_new_IDs (:1370) of a trivial, else 0; len1 / len2 / paired of vertex_read[v] in the store
                               the call found; visited = SRBuilder::visited after :1373; orientation = vertex_fwd[v]                   */
    /* per surviving super-read, single_SR_vec then paired_SR_vec (:1023-1024); room for n_pairs (+ 1 for the offsets) */
    hc_fno_read* srs;           /* id = the new id, len1 / len2 = the mates' lengths, paired                                            */
    uint32_t* sr_pair;          /* the pair it came from                                                                                */
    uint64_t* clique_off;       /* n_srs + 1 offsets into clique_nodes                                                                  */
    uint64_t* clique_nodes;     /* room for 4 n_pairs: get_sorted_clique(0) of a single (:864), get_sorted_clique(1) of a paired
                                   super-read (:853) — the vertex of every member of the pair's FIRST layout in member order (a paired
                                   read in an 's' layout appears twice) —, new_sorted_clique of a self-merged one (:913-935)            */
    uint64_t* subread_off;      /* n_srs + 1: 2 k                                                                                       */
    hc_fno_subread* subreads;   /* room for 2 n_pairs: the subreadMap (:857, :866), smaller vertex first; after a self-merge index2 +=
                                   overlap_pos where index2 >= 0 (:918-922)                                                            */
    uint32_t* tips;             /* room for n_vertices: the vertices of tips_vec in its order (:1302, :1309)                            */
    /* filled by the call */
    uint64_t n_srs, n_singles, n_trivials, n_paired, n_tips, n_self_merged;
    uint64_t new_read_count;    /* SRBuilder::new_read_count, :1380                                                                     */
    hc_sr_next_counts counts;   /* of the store: n_kept = new_read_count; the dropped counts over pairs and vertices together          */
    hc_sr_self_stats self_stats;
    double ms_device;           /* device call only: this section's own kernels, by events on the context's stream                     */
    double ms_copy;             /* device call only: waiting for the copies of the inputs and of the tables                             */
} hc_sr_merge_next_output;

/* Needs hc_sr_keep_device on, a store whose raw arrays were kept and kept consensus bytes (HC_ERR_STATE otherwise);
 * n_pairs + n_vertices >= 2^31, first_layout[n_pairs] > 2 n_pairs or n_members > 6 n_pairs: HC_ERR_ARG.  Any error leaves the old store usable.
 * 1. The super-read of pair i (:981-1001).  pair_status != HC_SR_EDGE_OK: none.  One layout: single-end, its bytes at out_off of that
 *    layout; two: paired.  An empty mate drops it.  A paired super-read with two non-empty mates goes through merge_self_overlap —
 *    hc_sr_merge_self_overlaps_kept's own run on an hc_sr_pair list built from out_off — and a merged pair becomes a single-end
 *    super-read at the offset the kept form appended it (the kept bytes grow as there).  Then test_N_rate.
 *    Refused as HC_SR_MN_NONE, nothing read: a vertex >= n_vertices, v == w, another number of layouts than 1 or 2, a layout or a
 *    member range outside the arrays, a first layout with no member or more than 4, descending out_off.
 * 2. visited[x] = 1 for both vertices of every super-read that survived 1, and only those (:1261-1277).  Two pairs naming one vertex
 *    both mark it.
 * 3. Every unvisited vertex in vertex order (:1282-1373), tested in the order of HC_SR_MN_V_*; a trivial has rev = !vertex_fwd[v]
 *    (:1331-1368).
 * 4. Ids: the single-end super-reads in pair order from 0 (a self-merged pair at its pair's place), then the trivials in vertex
 *    order, then the paired super-reads in pair order: hc_sr_set_next_reads' own numbering for that entry list.
 * 5. The store is replaced exactly as hc_sr_set_next_reads replaces it for that entry list (the same code from the gather on).  When
 *    nothing survives: HC_SR_NEXT_EMPTY, the outputs filled, the old store kept.
 * 6. After a self-merge (:911-935) the merged read's sorted clique lists, for each of the pair's two vertices, (vertex, index1) and,
 *    where index2 >= 0, (vertex, index2 + overlap_pos), ordered by index; among equal indexes the vertex of the first layout's SECOND
 *    member comes first, and a vertex's index1 entry before its index2 entry (the unordered_map's iteration order — the reverse of the
 *    insertion order of :571 for two keys — kept by the insertion sort std::sort is on four elements).
 * The member-to-vertex choice: a member is the smaller vertex's when its read is vertex_read of the smaller vertex, else the larger's.
 * The tables can be handed to hc_fno1_input as they are.  No base or quality byte crosses the link apart from the mates of the pairs the
 * host decides in the self-overlap scan. */
int hc_sr_merge_next(hc_ctx* ctx, const hc_sr_merge_next_input* in, const hc_sr_merge_next_settings* st, hc_sr_merge_next_output* out);

/* The same contract on the host (no device, no context): the current store as hc_set_reads takes it, the kept consensus bytes (n_cons
 * each), in, st, out — and the four arrays of the next store as hc_host_sr_next_reads returns them (out_seq_off: room for
 * 2 (n_pairs + n_vertices) + 1, out_read_first_seq: n_pairs + n_vertices + 1; cap / *n_bytes: count, then fetch).  It walks the
 * reference's loops as written, over hc_host_sr_merge_self_overlaps and hc_host_sr_next_reads.  ec_settings: --mismatch and
 * --min_read_len for the self-overlap test, as hc_host_sr_merge_self_overlaps takes them. */
int hc_host_sr_merge_next(const hc_settings* ec_settings, const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off,
                          const uint32_t* read_first_seq, uint32_t n_reads, const uint8_t* cons_seq, const uint8_t* cons_qual, uint64_t n_cons,
                          const hc_sr_merge_next_input* in, const hc_sr_merge_next_settings* st, hc_sr_merge_next_output* out,
                          uint8_t* out_bases, uint8_t* out_quals, uint64_t cap, uint64_t* n_bytes, uint64_t* out_seq_off,
                          uint32_t* out_read_first_seq);

/* ---- the rest of cliquesToSuperreads in one call: marks, trivials, the next store and the FNO tables -----------------------
 *
 * Between hc_sr_clique_merge and find-next-overlaps SRBuilder::cliquesToSuperreads (src/SRBuilder.cpp:1031-1235) judges the super-reads
 * (process_cliques, :981-1001, with merge_self_overlap, :872-955), marks the vertices of the survivors (:1122-1136), walks the unvisited
 * vertices for the trivial super-reads (:1145-1222; length, then N rate: this function has no inclusion and no tip test) and numbers
 * the three groups (:1141-1142, :1219-1220, :1233).  hc_sr_clique_next does that on the device from what hc_sr_clique_merge returned,
 * as hc_sr_merge_next does for an edge merge: it leaves the next store in the context and returns the tables of an hc_fno1_input.
 * The semantics are the reference's with N_THREADS = 1: with more threads process_cliques concatenates per-thread blocks in arrival
 * order (:1004-1011), which is not deterministic; one thread gives clique order.
 * Left to the caller: the text of cliques.txt (the cliques: hc_graph_cliques, include/hcedge.h; the gate behind the file:
 * hc_host_sr_clique_select).  The FASTQ text of the
 * new store: hc_sr_fastq_write_text, the last section.  The original-index maps (:750-806, :1161-1216) and subreads.txt: hc_sr_originals_next, below, on this call's outputs. */

typedef struct hc_sr_clique_next_input {
    /* what hc_sr_clique_merge took and returned, unchanged: host arrays */
    const uint64_t* clique_off;         /* n_cliques + 1; N = clique_off[n_cliques]                                                     */
    const uint32_t* clique_nodes;       /* N vertices, in any order inside a clique: process_cliques' clique_vec, :980                  */
    uint64_t n_cliques;
    const uint32_t* clique_status;      /* HC_SR_EDGE_* / HC_SR_CLIQUE_*: anything but HC_SR_EDGE_OK owns no super-read                 */
    const uint64_t* first_layout;       /* n_cliques + 1: one layout = single-end, two = paired (:850-869)                              */
    const hc_sr_layout* layouts;        /* first_layout[n_cliques] of them                                                              */
    const hc_sr_member* members;        /* not read: the rows come from member_vertex, the bytes from out_off.  May be NULL.            */
    const uint32_t* member_vertex;      /* n_members: sorted_vertices1 / sorted_vertices2 — the FULL lists set_sorted_clique keeps      */
    uint64_t n_members;                 /* at most 2 N, what hc_sr_clique_merge has room for (HC_ERR_ARG beyond)                        */
    const uint32_t* status;             /* HC_SR_* per layout: a layout that is not HC_SR_OK is an empty mate (:983, :999)              */
    const uint64_t* out_off;            /* n_layouts + 1: cons_seq1 / cons_seq2 (:852, :863) among the KEPT consensus bytes             */
    const hc_sr_subread_info* subreads; /* N: per clique its vertices' entries in ASCENDING VERTEX order, as hc_sr_clique_merge writes  */
    /* the graph's vertices */
    const uint32_t* vertex_read;        /* OverlapGraph::vertex_to_read as store indices, :1147                                         */
    const uint8_t* vertex_fwd;          /* OverlapGraph::getOrientation, :1180                                                          */
    uint64_t n_vertices;                /* OverlapGraph::getVertexCount, :1054, :1145                                                   */
} hc_sr_clique_next_input;

typedef struct hc_sr_clique_next_settings {
    uint32_t keep_singletons; /* program_settings.keep_singletons, :1149                                                    */
    uint32_t no_self_overlap; /* 1: merge_self_overlap (:985) is left out, every paired super-read stays paired             */
    hc_sr_self_settings self; /* merge_self_overlap's constants (:873-874: min_score 0.99, min_overlap 15) and minQual      */
} hc_sr_clique_next_settings; /* 32 bytes */

typedef struct hc_sr_clique_next_output {
    /* per clique (n_cliques entries each) */
    uint32_t* clique_kind;   /* HC_SR_MN_*                                                                                              */
    int32_t* clique_new_id;  /* Read id of the clique's super-read in the next store (:1142, :1233) or -1                               */
    int32_t* overlap_pos;    /* merge_self_overlap's overlap_pos (:882) of a clique it merged, else -1                                  */
    double* self_score;      /* overlap_score's value there (:886), else 0                                                              */
    /* per vertex (n_vertices entries each) */
    uint32_t* vertex_state;  /* HC_SR_MN_V_MERGED, _TRIVIAL, _SHORT, _N_RATE or _BAD                                                    */
    hc_fno_read* nodes;      /* as hc_sr_merge_next_output.nodes (id: nodes_to_new_IDs, :1219; visited: SRBuilder::visited after :1222) */
    /* per surviving super-read, single_SR_vec then paired_SR_vec (:1023-1024); room for n_cliques (+ 1 for the offsets) */
    hc_fno_read* srs;           /* id = the new id, len1 / len2 = the mates' lengths, paired                                            */
    uint32_t* sr_clique;        /* the clique it came from                                                                              */
    uint64_t* clique_off;       /* n_srs + 1 offsets into clique_nodes                                                                  */
    uint64_t* clique_nodes;     /* room for 2 N: get_sorted_clique(0) of a single (:864), get_sorted_clique(1) of a paired super-read
                                   (:853) — member_vertex of the clique's FIRST layout in member order —, new_sorted_clique of a
                                   self-merged one (:913-935) in the order stated below                                                */
    uint64_t* subread_off;      /* n_srs + 1 offsets into subreads                                                                      */
    hc_fno_subread* subreads;   /* room for N: the subreadMap (:857, :866), one entry per clique vertex in ascending vertex order;
                                   after a self-merge index2 += overlap_pos where index2 >= 0 (:918-922)                               */
    /* filled by the call */
    uint64_t n_srs, n_singles, n_trivials, n_paired, n_self_merged;
    uint64_t new_read_count;    /* SRBuilder::new_read_count, :1234                                                                     */
    hc_sr_next_counts counts;   /* of the store: n_kept = new_read_count; the dropped counts over cliques and vertices together        */
    hc_sr_self_stats self_stats;
    double ms_device;           /* device call only: this section's own kernels, sorts and scans, by events on the context's stream    */
    double ms_copy;             /* device call only: waiting for the copies of the inputs and of the tables                             */
} hc_sr_clique_next_output;

/* Needs hc_sr_keep_device on, a store whose raw arrays were kept and kept consensus bytes (HC_ERR_STATE otherwise).  HC_ERR_ARG:
 * n_cliques + n_vertices >= 2^31 or N >= 2^31; clique_off that does not start at 0 or descends; first_layout[n_cliques] > 2 n_cliques;
 * n_members > 2 N; the first layouts of the cliques that own a super-read (below) do not name ascending, disjoint member ranges in
 * clique order (hc_sr_clique_merge packs them so; the owner of a member is found by bisection).  Any error leaves the old store usable.
 * 1. The super-read of clique i (:981-1001).  clique_status != HC_SR_EDGE_OK: none.  One layout: single-end, its bytes at out_off of
 *    that layout; two: paired.  A layout that is not HC_SR_OK, or an empty mate, drops it.  A paired super-read with two non-empty mates
 *    goes through merge_self_overlap — hc_sr_merge_self_overlaps_kept's own run — and a merged one becomes the single-end read the kept
 *    form appended (the kept bytes grow as there).  Then test_N_rate.  The kinds are HC_SR_MN_*.
 *    Refused as HC_SR_MN_NONE, nothing read: a clique vertex or a vertex of the first layout's members >= n_vertices, fewer than two
 *    vertices, another number of layouts than 1 or 2, a layout or a member range outside the arrays, descending first_layout or out_off.
 * 2. visited[x] = 1 for every x of member_vertex of the FIRST layout of every super-read that survived 1, and only those (:1122-1136):
 *    the full list, whatever member_used says (set_sorted_clique keeps sorted_vertices1, :853, :864).  Cliques may overlap.
 * 3. Every unvisited vertex in vertex order (:1145-1222): HC_SR_MN_V_SHORT, then HC_SR_MN_V_N_RATE, else a trivial with
 *    rev = !vertex_fwd[v] (:1180-1217).
 * 4. Ids: the single-end super-reads in clique order from 0 (a self-merged clique at its clique's place), then the trivials in vertex
 *    order, then the paired super-reads in clique order: hc_sr_set_next_reads' own numbering for that entry list, and the store is
 *    replaced exactly as it replaces it (the same code from the gather on).  When nothing survives: HC_SR_NEXT_EMPTY, the outputs
 *    filled, the old store kept.
 * 5. After a self-merge (:911-935) every index2 >= 0 becomes index2 + overlap_pos, and the row lists, for each member of the first
 *    layout, (vertex, index1) and, where the vertex's index2 >= 0, (vertex, new index2), ordered by index.  The order among EQUAL
 *    indexes is this call's own: the entries are laid out by DESCENDING position of the vertex in the first layout's member list, a
 *    vertex's index1 entry before its index2 entry, and then sorted by index with a stable sort.  For a clique of two this is
 *    hc_sr_merge_next's documented order, which is the reference's; for more vertices the reference's order is the unordered_map's
 *    iteration followed by an unstable std::sort, and find-next-overlaps does not read it (FindNextOverlaps.cpp:900-913 pushes one
 *    pointer per listed vertex: membership with multiplicity is all that counts).
 * A clique list of two-vertex cliques gives exactly what hc_sr_merge_next gives for the same pairs with ignore_inclusions =
 * store_tips_separately = 0: every shared output and the store.
 * The tables can be handed to hc_fno1_input as they are.  The work is a fixed number of launches whatever the sizes: a lane per clique
 * vertex, clique, member, super-read or index entry, the owners by bisection, one stable radix sort of clique << 32 | vertex (so the
 * caller's cliques need not be sorted) and one of super-read << 32 | (index + 2^31) over all self-merged cliques' entries. */
int hc_sr_clique_next(hc_ctx* ctx, const hc_sr_clique_next_input* in, const hc_sr_clique_next_settings* st, hc_sr_clique_next_output* out);

/* The same contract on the host (no device, no context): the current store as hc_set_reads takes it, the kept consensus bytes (n_cons
 * each), in, st, out — and the four arrays of the next store as hc_host_sr_next_reads returns them (out_seq_off: room for
 * 2 (n_cliques + n_vertices) + 1, out_read_first_seq: n_cliques + n_vertices + 1; cap / *n_bytes: count, then fetch).  It walks the
 * reference's loops as written, over hc_host_sr_merge_self_overlaps and hc_host_sr_next_reads. */
int hc_host_sr_clique_next(const hc_settings* ec_settings, const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off,
                           const uint32_t* read_first_seq, uint32_t n_reads, const uint8_t* cons_seq, const uint8_t* cons_qual, uint64_t n_cons,
                           const hc_sr_clique_next_input* in, const hc_sr_clique_next_settings* st, hc_sr_clique_next_output* out,
                           uint8_t* out_bases, uint8_t* out_quals, uint64_t cap, uint64_t* n_bytes, uint64_t* out_seq_off,
                           uint32_t* out_read_first_seq);

/* The gate in front of process_cliques (src/SRBuilder.cpp:1056-1084) over the cliques of cliques.txt in file order, as a CSR: with
 * remove_multi_occ a clique first loses the vertices that an earlier ACCEPTED clique used (:1065-1073); what is left counts as a
 * singleton when it has one vertex (:1075-1077) and is accepted when it has at least min_clique_size (:1078-1084; used_nodes is set on
 * acceptance only, and whatever remove_multi_occ says).  A clique left with no vertex is neither (with min_clique_size == 0 it is
 * accepted, as the reference accepts it).  Serial by definition — every clique sees the ones accepted before it — and host only.
 * Outputs: sel_off (room for n_cliques + 1) / sel_nodes (room for clique_off[n_cliques]): the accepted cliques, filtered, in file
 * order; sel_index (room for n_cliques): the index of each in the input; *n_selected; *n_singletons.
 * HC_ERR_ARG: a null array, clique_off that does not start at 0 or descends, a vertex >= n_vertices (the reference's bitset asserts). */
int hc_host_sr_clique_select(const uint64_t* clique_off, const uint32_t* clique_nodes, uint64_t n_cliques, uint64_t n_vertices,
                             uint32_t min_clique_size, int remove_multi_occ, uint64_t* sel_off, uint32_t* sel_nodes, uint64_t* sel_index,
                             uint64_t* n_selected, uint64_t* n_singletons);

/* ---- the original-read index maps on the device, and subreads.txt ----------------------------------------------------------
 *
 * OverlapGraph::original_ID_dict (src/OverlapGraph.cpp:768-846) is the one table the reference carries from an iteration to the next
 * through a file: per read of the store, the reads of the FIRST iteration it is made of, each with its place in it.  constructSuperread
 * folds the maps of a clique's reads into the super-read's (src/SRBuilder.cpp:750-806), merge_self_overlap shifts them (:938-949), a
 * trivial super-read copies or reverses its read's (:1161-1216, :1312-1369), and the three writers append one line per new read to
 * subreads.txt (:1449-1463, :1489-1503, :1537-1551).  Here the dict stays in the context: a CSR over the reads of a store,
 * orig_off[n_reads + 1] + entries.
 * Two things are this project's own.  (1) The reference's order inside a map, and inside a line, is libstdc++'s unordered_map
 * iteration order; every reader puts the entries back into a map.  Here the entries of a read are in ASCENDING ORIGINAL ID, in the
 * arrays and in the text.  (2) index2 / len2 of a single-end original are never set nor printed by the reference: here they are 0 on
 * output and ignored on input.
 * FNO=3, which reads the dict: hc_fno3_from_originals, behind this section's functions.  (BranchReduction's read evidence:
 * hc_br_evidence, the section behind that one; the FASTQ text: hc_sr_fastq_write_text, the section after that.) */

typedef struct hc_sr_original {
    uint32_t id;            /* the original read's id                                                                   */
    int32_t index1, index2; /* OriginalIndex::index1 / index2 (long there; a result outside int32 is HC_SR_ORIG_RANGE)  */
    uint32_t len1, len2;    /* OriginalIndex::len1 / len2                                                               */
    uint8_t paired;         /* OriginalIndex::is_paired                                                                 */
    uint8_t forward;        /* OriginalIndex::forward                                                                   */
    uint8_t pad[2];         /* 0                                                                                        */
} hc_sr_original; /* 24 bytes */

/* Per read of the new dict.  A read that is not OK has no entries. */
enum {
    HC_SR_ORIG_OK = 0,
    HC_SR_ORIG_EMPTY_SOURCE = 1,   /* a trivial super-read whose read has an empty map: assert (subreads.size() > 0), :1178, :1329 */
    HC_SR_ORIG_SEQ0_OF_PAIRED = 2, /* :801 calls get_seq(0) on a paired sub-read (a single-end original under a reverse vertex of a
                                      paired read, not first_it): the assert of src/Read.h:145-149                                */
    HC_SR_ORIG_RANGE = 3           /* an index left int32 (with HC_SR_ORIG_SEQ0_OF_PAIRED in the same read, that one is reported) */
};
/* hc_sr_originals_next: HC_OK is 0; reads with a status other than OK are no error of the arguments. */
#define HC_SR_ORIG_SOME_FAILED 1

/* What hc_sr_merge_next or hc_sr_clique_next returned and took, for both: an edge merge is the clique list with two vertices per pair
 * (kind = pair_kind, new_id = pair_new_id, sr_clique = sr_pair). */
typedef struct hc_sr_originals_input {
    /* per source clique / pair (n_cliques entries; first_layout: n_cliques + 1) */
    const uint32_t* kind;         /* HC_SR_MN_*: HC_SR_MN_SINGLE_SELF means merge_self_overlap merged it, :938-949                  */
    const int32_t* new_id;        /* the super-read's id in the next store                                                         */
    const int32_t* overlap_pos;   /* read for HC_SR_MN_SINGLE_SELF only                                                            */
    const uint64_t* first_layout; /* two layouts: the second one's total_len is constructSuperread's len2 (:693, :788), else 0     */
    uint64_t n_cliques;
    const hc_sr_layout* layouts;
    /* per surviving super-read */
    const uint32_t* sr_clique;       /* the clique it came from                                                                    */
    const uint64_t* subread_off;     /* n_srs + 1                                                                                  */
    const hc_fno_subread* subreads;  /* per super-read its vertices in ASCENDING VERTEX order, the loop order of :752; index2 as the
                                        merge call returned it (shifted after a self-merge: the call undoes that)                  */
    uint64_t n_srs;
    /* per vertex */
    const uint32_t* vertex_state; /* HC_SR_MN_V_*: HC_SR_MN_V_TRIVIAL owns the new read nodes[v].id                                */
    const hc_fno_read* nodes;     /* id of a trivial; len1 / len2 / paired of vertex_read[v] in the store the merge call found     */
    const uint32_t* vertex_read;  /* indexes the kept dict                                                                         */
    const uint8_t* vertex_fwd;
    uint64_t n_vertices;
    uint64_t new_read_count;      /* reads of the new dict                                                                         */
    uint32_t first_it;            /* program_settings.first_it, :767                                                               */
    uint32_t reserved;
} hc_sr_originals_input;

typedef struct hc_sr_originals_output {
    uint64_t* orig_off; /* room for new_read_count + 1: the new dict's offsets                    */
    uint32_t* status;   /* room for new_read_count: HC_SR_ORIG_*                                  */
    uint64_t n_entries; /* entries of the new dict                                                */
    uint64_t n_failed;  /* reads whose status is not HC_SR_ORIG_OK                                */
    double ms_device;   /* device call only: kernels, sort and scans, by events on the stream     */
    double ms_copy;     /* device call only: waiting for the copies of the inputs and the results */
} hc_sr_originals_output;

typedef struct hc_sr_originals_text_counts {
    uint64_t n_bytes, n_lines;
    double ms_device;
} hc_sr_originals_text_counts;

/* buildOriginalsDict with first_it (src/OverlapGraph.cpp:772-797) for the context's current store: read r gets the one entry
 * (r, index1 = 0, forward, len1) and, paired, (index2 = 0, len2, paired).  One lane per read, the lengths from the store's
 * descriptors.  HC_ERR_STATE: no store. */
int hc_sr_originals_init(hc_ctx* ctx);

/* Makes the caller's dict the kept one.  HC_ERR_STATE: no store; HC_ERR_ARG: n_reads is not the current store's number of reads,
 * orig_off does not start at 0 or descends, 2^31 entries or more, ids that do not strictly ascend inside a read, paired or forward
 * above 1.  A read with no entry is allowed (hc_sr_originals_next reports it where the reference asserts).  index2 / len2 of a
 * single-end entry are stored as 0.  Any error leaves the kept dict as it was. */
int hc_sr_originals_load(hc_ctx* ctx, const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads);

/* The kept dict.  *n_reads / *n_entries are always filled (0 and HC_ERR_STATE when none is kept).  cap_reads = entries orig_off has
 * room for beyond its first, cap_entries = room of entries; where either is too small or a buffer is NULL nothing is copied and
 * HC_ERR_ARG is returned (count, then fetch). */
int hc_sr_originals_fetch(hc_ctx* ctx, uint64_t* orig_off, uint64_t cap_reads, hc_sr_original* entries, uint64_t cap_entries,
                          uint64_t* n_reads, uint64_t* n_entries);

/* The dict of the NEXT store from the kept dict of the store the merge call found, which it then replaces.  It may run after the merge
 * call has replaced the store: what it needs of the old reads is in `nodes`.
 * New read new_id[c] of a surviving super-read k (c = sr_clique[k]; :750-806): its vertices in the order of `subreads`; for vertex v
 * every entry e of the dict of vertex_read[v] whose id no earlier vertex supplied, with
 *     fwd = vertex_fwd[v], i2 = the row's index2 before the self-merge shift, idx1 = index1 - startpos1, idx2 = i2 - startpos2,
 *     e.forward = (e.forward == fwd), and
 *     first_it:  e.index1 = idx1; paired e: e.index2 = idx2                                                            (:767-772)
 *     fwd:       e.index1 += idx1; paired e: e.index2 += i2 >= 0 ? idx2 : idx1                                         (:773-783)
 *     else, paired e, paired read:  e.index1 = len1(v) + idx1 - (e.len1 + e.index1),
 *                                   e.index2 = len2(v) + (len2 > 0 || i2 >= 0 ? idx2 : idx1) - (e.len2 + e.index2)     (:786-794)
 *           paired e, single read:  e.index1 = len1(v) + idx1 - (e.len1 + e.index1), e.index2 = len1(v) + idx1 - (e.len2 + e.index2)
 *           single e, single read:  e.index1 = len1(v) + idx1 - (e.len1 + e.index1)                                    (:801)
 *           single e, paired read:  HC_SR_ORIG_SEQ0_OF_PAIRED
 *     HC_SR_MN_SINGLE_SELF: paired e: e.index2 += overlap_pos                                                          (:938-949)
 * New read nodes[v].id of a trivial v (:1161-1216, :1312-1369): the dict of vertex_read[v] as it is for a forward vertex; for a reverse
 * one forward is flipped, index1 = L1 - (index1 + len1) and, for a paired read, index2 = L2 - (index2 + len2), for a paired e in a
 * single-end read index2 = L1 - (index2 + len2) (L1 / L2 = nodes[v].len1 / len2); an empty dict is HC_SR_ORIG_EMPTY_SOURCE.
 * A status is decided by the entries that WIN (an entry the reference skips at :762 asserts nothing).
 * HC_ERR_STATE: no kept dict.  HC_ERR_ARG: a null array, a subread row's node >= n_vertices, vertex_read[v] of such a vertex or of a
 * trivial not below the kept dict's reads, sr_clique >= n_cliques, a new id not below new_read_count, descending subread_off,
 * new_read_count or the candidate entries 2^31 or more.  Any error leaves the kept dict in place; HC_SR_ORIG_SOME_FAILED replaces it.
 * A fixed number of launches whatever the sizes: a lane per source (a super-read's vertex, or a vertex) for its dict's length, one
 * exclusive sum, a lane per candidate entry (its source by bisection) for the transform and the key new id << 32 | original id, one
 * stable radix sort — among equal keys the smallest vertex stays first, the reference's winner —, the first of every run, one ordered
 * selection, a gather, and the offsets by bisection. */
int hc_sr_originals_next(hc_ctx* ctx, const hc_sr_originals_input* in, hc_sr_originals_output* out);

/* The bytes of subreads.txt for the kept dict, on the device until the next hc_sr_originals_write_text or the next call that replaces
 * the dict: line k is read k — "k", then per entry "\tID:+:index1:len1" or "\tID:-:index1,index2:len1,len2", then "\n" (:1449-1463) —
 * entries in ascending original id.  hc_sr_originals_text_fetch copies bytes [first, first + count) out (a range outside the text:
 * HC_ERR_ARG; no text: HC_ERR_STATE). */
int hc_sr_originals_write_text(hc_ctx* ctx, hc_sr_originals_text_counts* counts);
int hc_sr_originals_text_fetch(hc_ctx* ctx, uint64_t first, uint64_t count, char* dst);

/* The same contracts on the host (no device, no context): the loops of the cited lines as written, then every map sorted by id.
 * hc_host_sr_originals_next: the old dict (n_reads reads) in, the new one out — out_entries: room for cap entries; *out->n_entries is
 * always filled, too small a cap or NULL: HC_ERR_ARG with the offsets and statuses filled (count, then fetch).  n_threads: super-reads
 * and trivials are independent (0 or 1: one thread). */
int hc_host_sr_originals_next(const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads, const hc_sr_originals_input* in,
                              hc_sr_originals_output* out, hc_sr_original* out_entries, uint64_t cap, uint32_t n_threads);
/* text: room for cap bytes; *n_bytes always filled (count, then fetch). */
int hc_host_sr_originals_text(const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads, char* text, uint64_t cap,
                              uint64_t* n_bytes);
/* buildOriginalsDict's else branch (src/OverlapGraph.cpp:807-838) on the bytes of a subreads.txt: a line is split at tabs, its first
 * field is the read's id, every further field is split at ':' and ',' with adjacent separators taken as one, 4 tokens = single-end,
 * 6 = paired; original_ID_dict.insert keeps the FIRST line of an id and a map the first entry of an original id.  The dict has
 * max id + 1 reads.  *n_reads / *n_entries always filled; cap_reads / cap_entries as hc_sr_originals_fetch.  HC_ERR_FORMAT, with
 * *bad_line = the 0-based line: a field of another token count than 4 or 6 (the assert of :816), or a token std::stol / stoi or
 * str_to_read_id would not take whole, or a value outside its type here. */
int hc_host_sr_originals_parse(const char* text, uint64_t n_bytes, uint64_t* orig_off, uint64_t cap_reads, hc_sr_original* entries,
                               uint64_t cap_entries, uint64_t* n_reads, uint64_t* n_entries, uint64_t* bad_line);

/* ---- FNO=3 from the kept dict: SRBuilder::findNextOverlaps3 on the device ----------------------------------------------------
 *
 * A clique iteration ends with findNextOverlaps3 (src/FindNextOverlaps3.cpp:20-173): every pair of reads of the new store that share an
 * original read becomes a candidate, deduceOverlap (:176-406) turns it into one line of the next overlaps.txt.  hc_fno3_run
 * (include/hcfno.h) walks the reference's unordered_map on the host, so that its lines come in the reference's order; this call reads
 * the kept dict and the store's read descriptors (len1, len2, paired; a read's id is its index) where they are and never leaves the
 * device.  The SET of candidate pairs is the reference's.  Two things are this call's own, because in the reference they follow
 * libstdc++'s hash iteration order:
 *  - the order of the lines: here ascending (walk rank of SR1, walk rank of SR2).  No reader depends on the file's order;
 *  - for a pair that shares several originals, which one deduceOverlap uses: here the shared one of SMALLEST ID.  deduceOverlap reads
 *    the chosen original through d_l = index1 in SR1 - index1 in SR2 and, when either read is paired, d_r = index2 in SR1 - index2 in
 *    SR2 (int32 arithmetic, as the reference's int) and nothing else.  A pair is AMBIGUOUS when two of its shared originals give
 *    different d_l (both reads single-end) or different (d_l, d_r) (otherwise); for every other pair the line is the reference's
 *    whatever the hash order was.  Ambiguous pairs are counted and flagged in the candidate table.
 * SR1 of a pair is the read of lower WALK RANK, the reference's i < j in SR_list: the place of a read in single_SR_vec ++
 * paired_SR_vec ++ trivial_SR_vec (:29-76).  The stores hc_sr_merge_next and hc_sr_clique_next build number the single-end
 * super-reads from 0, then the trivials, then the pairs, and each of the reference's three deques is in ascending id
 * (src/SRBuilder.cpp:1142-1233, :1280-1378, writeSinglesToFile / writePairsToFile number a deque front to back, the trivials are pushed
 * in the vertex order that numbers them), so walk_rank = NULL derives the rank from the three counts.  A paired super-read and a
 * trivial single-end read behind it form the P-S branch (:240-281) with the pair as SR1.
 * The tests of :157-165 apply as they are: with HC_FNO_NO_INCLUSIONS a pair whose get_perc() is 100 writes no line, nor does one with
 * len1 <= 0.  Whatever the reference would stop at (the assert of :391, the Overlap constructor's checks): HC_ERR_FORMAT, no text.
 * index2 of a single-end original is the dict's 0.
 * A fixed number of launches whatever the sizes, no atomics on the outputs, the same bytes on every run: a lane per dict entry (its
 * read by bisection) for the key original id << 32 | walk rank, one stable radix sort; the heads of the runs give n_originals and each
 * entry's combinations with the later entries of its run; one exclusive sum; a lane per combination (its entry by bisection) for the
 * key rank of SR1 << b | rank of SR2, b = bits of n_reads - 1, and (d_l, d_r); one stable radix sort over 2 b bits, which leaves the
 * smallest shared original first in every run; the heads of the runs are the candidates, one sum over "differs from its predecessor
 * in the run" read at the run boundaries marks the ambiguous ones; a lane per candidate fills the record hc_fno3_run's device form
 * takes, and deduceOverlap, the exclusive sum and the text are that form's kernels.
 * Memory: about 45 bytes per combination and the sort's scratch, in the context's blocks (grow-only).
 * The text and the candidate table stay on the device until the next hc_fno3_from_originals or the next call that replaces the dict or
 * the store (hc_sr_originals_write_text's rule; a store of another number of reads than the dict's is refused).
 * HC_ERR_STATE: no store, no kept dict, or a dict over another number of reads than the store's.  HC_ERR_ARG: a null argument, counts
 * that do not add up to the store's reads, a walk_rank that is no permutation, unknown bits in flags, max_combos above 2^31 - 16.
 * HC_ERR_FORMAT: more distinct originals than original_readcount (nodes_to_SR.at, :37), or a stop of the reference.
 * HC_ERR_NOT_ON_DEVICE: more than max_combos combinations — decided before anything of that size is allocated.  Every error leaves
 * the text and the table of the call before in place, HC_ERR_FORMAT apart (nothing is kept after it). */
typedef struct hc_fno3_resident_input {
    uint64_t n_single, n_trivial, n_paired; /* reads of the current store in id order: singles, trivials, pairs */
    const uint32_t* walk_rank;  /* optional [n_reads]: place of read r in single_SR_vec ++ paired_SR_vec ++ trivial_SR_vec
                                   (FindNextOverlaps3.cpp:29-76); a permutation.  NULL: derived from the three counts
                                   (single r -> r; pair r -> r - n_trivial; trivial r -> r + n_paired) */
    uint64_t original_readcount; /* more distinct originals than this: HC_ERR_FORMAT (nodes_to_SR.at, :37) */
    uint64_t max_combos;         /* 0 = 2^31 - 16; more (pair, original) combinations: HC_ERR_NOT_ON_DEVICE, nothing changed */
    uint32_t flags;              /* HC_FNO_NO_INCLUSIONS; other HC_FNO_KNOWN_FLAGS accepted and ignored as hc_fno3_run does; unknown bits HC_ERR_ARG */
    uint32_t reserved;
} hc_fno3_resident_input;

typedef struct hc_fno3_resident_counts {
    uint64_t n_lines, n_bytes;
    uint64_t candidates;   /* distinct pairs = overlaps_list.size(); equal to hc_fno3_run's counter on the same data */
    uint64_t n_combos;     /* (pair, shared original) combinations */
    uint64_t n_ambiguous;  /* pairs whose shared originals disagree (definition above) */
    uint64_t n_originals;  /* distinct original ids in the dict */
    double ms_device;      /* device call only: kernels, sorts and sums, by events on the stream */
} hc_fno3_resident_counts;

#define HC_FNO3_CAND_AMBIGUOUS 0x1u
#define HC_FNO3_CAND_LINE      0x2u
/* One candidate pair, in the order of the lines.  a, b: the reads (their index in the store = their id there; the mirror: their index
 * in `reads`), rank(a) < rank(b); original_id: the shared original the line is deduced from. */
typedef struct hc_fno3_candidate {
    uint32_t a, b;
    uint32_t original_id;
    uint32_t flags; /* HC_FNO3_CAND_AMBIGUOUS | HC_FNO3_CAND_LINE (it wrote a line) */
} hc_fno3_candidate; /* 16 bytes */

int hc_fno3_from_originals(hc_ctx* ctx, const hc_fno3_resident_input* in, hc_fno3_resident_counts* counts);
/* Bytes [first, first + count) of the text / candidates [first, first + count) of the table.  A range outside what is kept:
 * HC_ERR_ARG; nothing kept: HC_ERR_STATE. */
int hc_fno3_text_fetch(hc_ctx* ctx, uint64_t first, uint64_t count, char* dst);
int hc_fno3_candidates_fetch(hc_ctx* ctx, uint64_t first, uint64_t count, hc_fno3_candidate* dst);

/* The same rule on the host (no device, no context), as loops over plain arrays: the dict over n_reads reads, reads[r] = id (what the
 * lines print; any distinct labels), len1, len2, paired of read r; in as above, with the counts adding up to n_reads.  *counts is
 * always filled (ms_device 0), *n_bytes too; text: room for cap bytes, cands: room for cap_cands candidates — where either is NULL or
 * too small nothing is copied and HC_ERR_ARG is returned (count, then fetch).  HC_ERR_ARG also for a read of length 0. */
int hc_host_fno3_from_originals(const uint64_t* orig_off, const hc_sr_original* entries, uint64_t n_reads, const hc_fno_read* reads,
                                const hc_fno3_resident_input* in, hc_fno3_resident_counts* counts, char* text, uint64_t cap,
                                uint64_t* n_bytes, hc_fno3_candidate* cands, uint64_t cap_cands);

/* ---- read evidence for branching edges: the first half of BranchReduction::readBasedBranchReduction -------------------------
 *
 * POLYTE runs every iteration with --branch_reduction, so its branch step is readBasedBranchReduction (src/ViralQuasispecies.cpp:326-347,
 * src/BranchReduction.cpp:41-227).  Its first half — findBranchingEvidence with buildDiffListOut, buildDiffListIn, findDiffPos and
 * checkReadEvidence (:229-743), called for every in-branch and then every out-branch (:60-80) — reads the cleaned graph, the store's
 * sequences, the original-read index maps and the reads of --original_fastq, and every result of it is independent of hash iteration
 * order because the lists are sorted before use.  hc_br_evidence computes it on the device from what the context holds.  The second half
 * (findBranchingComponents, countUniqueEvidence, the threshold file and the removals, :82-227 and :745-1272) is hc_br_reduce, the
 * section behind this one: it walks unordered_maps in iteration order, and its result depends on that order, so that walk runs on the
 * host in real libstdc++ maps and only the order-free part — the unique-evidence filter and the graph edit — runs on the device.
 *
 * A branch is a vertex with more than one in-neighbour (side HC_BR_IN) or more than one out-neighbour (HC_BR_OUT); its neighbours are
 * sortAdjLists(adj_in) / sortAdjOut(adj_out) (:47-48), ascending.  The edge of a neighbour is getEdgeInfo's: the FIRST record
 * node1 -> node (out) / node -> node1 (in) in list order after sortAdjOut; pos = its pos1, the neighbour's read = its read2 (out) /
 * read1 (in), an index into the store.  The reference indexes original_ID_dict by vertex, which is the read wherever --add_duplicates
 * is off; HERE THE DICT OF VERTEX v IS THE DICT OF READ vertex_read[v].  vertex_read / vertex_fwd mean what they mean for
 * hc_sr_edge_merge (getOrientation(v) = vertex_fwd[v]).
 *
 * Restated as the reference has it:
 *  - every neighbour sequence takes the orientation of node1, not its own (:414, :556); a reverse node1 reads the neighbour's stored
 *    bytes back to front through build_rev_comp's mapping (a byte build_rev_comp exits on stays as it is);
 *  - an in-branch compares its pairs from the back and records len - pos + startpos (:627), one beyond the position it found;
 *  - result2 re-checks the sub-read itself: it differs from result1 only in which id must be in subreads1 (:304-321);
 *  - the joint id is original_readcount + min(id, mate id) (:318);
 *  - read_end uses the ORIGINAL read's full length, not the entry's len1 (:720);
 *  - int(seq.size() - min_overlap_len) is a 64-bit difference cut to 32 bits (:449, :461, :605, :616);
 *  - dist = 0.5 * (min + max) assigned to an int: it truncates toward zero (:521-530, :675-684);
 *  - with exactly two neighbours and a missing inclusion pair final_branch is cleared (:330-332); the ++ on its begin() at :349 then
 *    lands on end() in libstdc++, so nothing is stored for the branch;
 *  - checkReadEvidence's early break (:733-737) makes its result "no covered position disagrees and at least one is covered", which does
 *    not depend on the walk's order; the covered positions are one contiguous range of the sorted diff list;
 *  - pos3 / pos4 of a missing edge are never set by the reference (src/Edge.h:41-56): 0 here. */

enum { HC_BR_IN = 0, HC_BR_OUT = 1 };
/* Per branch: the reference's asserts on this path, checked in the reference's order (the first that fails is reported). */
enum {
    HC_BR_OK = 0,
    HC_BR_PAIRED_NEIGHBOUR = 1,   /* assert (!read->is_paired()), :412, :554                                                       */
    HC_BR_REPEATED_NEIGHBOUR = 2, /* assert (node_i != node_j), :446; the same pair in the in-branch loop is refused alike         */
    HC_BR_BAD_GEOMETRY = 3,       /* assert (len > 0), :471 / :625 (a relative position beyond the sequence included, where substr
                                     throws); the inclusion asserts of an in-branch, :605 / :616                                    */
    HC_BR_BAD_ORIGINAL = 4        /* get_read of a dict id that is no original read (:288, :306); the asserts :300 / :319         */
};
/* hc_br_evidence / hc_host_br_evidence: HC_OK is 0; branches with a status other than OK are no error of the arguments.  A failed branch
 * contributes nothing: no evidence, no missing edge, no false mark, an empty final_branch and diff list, dist 0. */
#define HC_BR_SOME_FAILED 1
#define HC_BR_MAX_DIFFS 100u /* findDiffPos keeps at most 100 positions per pair, :703 */

typedef struct hc_br_settings {
    uint64_t se_count, pe_count;  /* program_settings.branch_SE_c / branch_PE_c: originals are numbered singles, /1 mates, /2 mates  */
    uint64_t original_readcount;  /* program_settings.original_readcount (< 2^31)                                                    */
    uint32_t min_overlap_len;     /* program_settings.min_overlap_len                                                                */
    uint32_t reserved;            /* 0                                                                                               */
    double edge_threshold;        /* program_settings.edge_threshold: the score of a missing edge                                    */
} hc_br_settings; /* 40 bytes */

typedef struct hc_br_branch {
    uint32_t node;      /* the branching vertex                                                                                     */
    uint8_t side;       /* HC_BR_IN / HC_BR_OUT                                                                                     */
    uint8_t status;     /* HC_BR_*                                                                                                  */
    uint8_t is_false;   /* member of false_in_branches / false_out_branches (:513, :667)                                            */
    uint8_t pad;        /* 0                                                                                                        */
    int32_t dist;       /* the int of :521-530 / :675-684                                                                           */
    uint32_t nb_count;  /* final_branch without its front entry: branch_nb[nb_first, nb_first + nb_count); 0 where :330-332 cleared */
    uint64_t nb_first;
    uint64_t diff_first; /* the sorted, de-duplicated diff list (:532-533, :686-687): diff_pos[diff_first, diff_first + diff_count)  */
    uint32_t diff_count;
    uint32_t n_neighbours; /* neighbours.size()                                                                                      */
} hc_br_branch; /* 40 bytes */

typedef struct hc_br_counts {
    uint64_t n_branches;  /* records of `branches`: in-branches in ascending vertex, then out-branches in ascending vertex (:60-80) */
    uint64_t n_branch_nb; /* entries of branch_nb                                                                                   */
    uint64_t n_diff;      /* entries of diff_pos                                                                                    */
    uint64_t n_ev_edges;  /* keys of evidence_per_edge                                                                              */
    uint64_t n_ev_ids;    /* ids in all its lists                                                                                   */
    uint64_t n_missing;   /* missing_edges                                                                                          */
    uint64_t n_items;     /* (branch, neighbour, entry of the neighbour's dict) triples of the branches that reach the evidence loop */
    uint64_t n_failed;    /* branches whose status is not HC_BR_OK                                                                  */
    double ms_device;     /* device call only: the target-order step, kernels, sorts and sums by events on the context's stream     */
} hc_br_counts; /* 72 bytes */

/* Count, then fetch: every pointer may be NULL (not wanted); a wanted table whose cap is below its count: HC_ERR_ARG, nothing copied.
 *   branch_nb      the neighbours of every final_branch: the sorted list minus node_pair.first of every missing inclusion pair (:328-335)
 *   diff_pos       per branch its diff list
 *   ev_edge        evidence_per_edge's keys as pairs u, v (2 * cap_ev_edges entries) in ascending (u, v) — an edge is listed exactly when
 *                  the reference's map has its key, an empty list included —, ev_off (cap_ev_edges + 1) into ev_ids, ids ascending; an
 *                  edge stored from both its in-branch and its out-branch holds the intersection (:367-384)
 *   missing_edges  (:476-511, :630-665) in push order: branches as above, pairs in (i, j) order; score = edge_threshold, pos1 = relative_pos, pos2 = 0,
 *                  ord '-', ori1 / ori2 / read1 / read2 / v1 / v2 by :489-506 / :643-660, perc by the integer division of :487 / :641,
 *                  len0 = len1 = len, len2 = 0, mismatch_rate = -1, pos3 = pos4 = 0 */
typedef struct hc_br_tables {
    hc_br_branch* branches;
    uint64_t cap_branches;
    uint32_t* branch_nb;
    uint64_t cap_branch_nb;
    int32_t* diff_pos;
    uint64_t cap_diff;
    uint32_t* ev_edge;
    uint64_t* ev_off;
    uint64_t cap_ev_edges;
    uint32_t* ev_ids;
    uint64_t cap_ev_ids;
    hc_edge_rec* missing_edges;
    uint64_t cap_missing;
} hc_br_tables; /* 104 bytes */

/* The sequences of --original_fastq as FastqStorage holds them: single-end (src/ViralQuasispecies.cpp:328-334), one byte per base,
 * n_reads + 1 ascending offsets from 0.  They stay on the device until replaced or hc_reset.  HC_ERR_ARG: a null array, offsets that
 * do not start at 0 or descend, 2^32 reads or more. */
int hc_br_set_original_reads(hc_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint64_t n_reads);

/* findBranchingEvidence for every branch of the graph the context holds.  HC_ERR_STATE unless the context has a graph (not one with
 * hc_graph_resolve's tied lists), a store loaded while hc_sr_keep_device was on, a kept dict with as many reads as the store, and
 * original reads.  HC_ERR_ARG: a null argument, n_vertices that is not the graph's, se_count + 2 * pe_count != the original reads (the
 * assert of src/ViralQuasispecies.cpp:341), original_readcount >= 2^31, a vertex_read that is no read of the store, a neighbour's record
 * whose read1 / read2 is no read of the store (checked for every neighbour, ahead of any status), 2^32 / 100 neighbour pairs or 2^31 items or more.
 * SIDE EFFECT ON THE GRAPH: adj_out is left in target order — sortAdjOut's side effect (:48, src/GraphAlgos.cpp:831), by the step
 * hc_graph_remove_branches uses, its host step for lists that repeat a target included.  Apart from that the graph is read, never
 * written: no edge is removed and branching_edges is not touched.
 * The tables stay on the device until the next hc_br_evidence, hc_graph_load / hc_graph_resolve, hc_set_reads or hc_reset; a fetch
 * after that: HC_ERR_STATE.
 * A fixed number of launches whatever the degrees and dict sizes (DESIGN.md §5 has the kernels): A — a lane per vertex and side, per
 * neighbour and per branch, then a WAVE per pair of neighbour sequences that walks the overlap 64 positions at a time and ranks the
 * differing lanes by ballot; B — per branch its status, dist and final_branch, one stable radix sort of branch << 32 | position for the
 * diff lists; C — a lane per item (branch, neighbour, dict entry) with binary searches of node1's dict and of the diff list, up to two
 * keys record << 33 | id << 1 | side; D — one stable sort of the keys, the intersection where both sides stored the edge, selections.
 * A branch that fails only in C (HC_BR_BAD_ORIGINAL) is known after B has laid its lists out: the call then runs B - D once more with
 * those branches failed (at most once: branches do not depend on one another). */
int hc_br_evidence(hc_ctx* ctx, const uint32_t* vertex_read, const uint8_t* vertex_fwd, uint64_t n_vertices, const hc_br_settings* settings,
                   hc_br_counts* counts);
/* The tables of the last hc_br_evidence (cap_* in the struct).  HC_ERR_STATE: none kept. */
int hc_br_evidence_fetch(hc_ctx* ctx, hc_br_tables* tables);

/* The same on the host (no device, no context), following the reference's loops: the yardstick for the device call.  The graph as
 * hc_graph_fetch returns it (adj_out in any order: the mirror sorts a copy as sortAdjOut does and leaves the caller's arrays alone), the
 * store's raw arrays as hc_set_reads takes them, the dict as hc_sr_originals_fetch returns it (over n_reads reads), the original reads
 * as hc_br_set_original_reads takes them.  counts is always filled; tables may be NULL (count, then fetch).  n_threads: branches are
 * independent (0 or 1: one thread). */
typedef struct hc_br_host_input {
    const hc_edge_rec* edges;
    const uint64_t* out_off;
    const uint32_t* in_nodes;
    const uint64_t* in_off;
    uint64_t n_vertices;
    const uint8_t* bases;
    const uint64_t* seq_off;
    const uint32_t* read_first_seq;
    uint64_t n_reads;
    const uint64_t* orig_off;
    const hc_sr_original* entries;
    const uint8_t* original_bases;
    const uint64_t* original_seq_off;
    uint64_t n_original_reads;
    const uint32_t* vertex_read;
    const uint8_t* vertex_fwd;
} hc_br_host_input; /* 128 bytes */
int hc_host_br_evidence(const hc_br_host_input* in, const hc_br_settings* settings, hc_br_counts* counts, hc_br_tables* tables,
                        uint32_t n_threads);

/* ---- the reduction: the second half of BranchReduction::readBasedBranchReduction ------------------------------------------------
 *
 * hc_br_reduce runs src/BranchReduction.cpp:82-227 with findBranchingComponents, extendComponentOut / In and countUniqueEvidence
 * (:745-1272) on the tables the last hc_br_evidence left on the device, and edits the device graph in place like every other cleaning
 * call: POLYTE's branch step is hc_br_evidence, hc_br_reduce and nothing else.
 *
 * What depends on unordered_map iteration order is small and serial and runs on the HOST, in std::unordered_map< node_id_t, ... >
 * objects that receive the reference's inserts in the reference's order (:753-781): which in-branch starts a component, the depth-first
 * walk, `dist` (:806-833, :906-925: from the starting branch and the last top-level neighbour the walk extended), the order of
 * branching_components that the --careful chain (:163-204) reads, and the tie order of the diploid rule's at most four (mapID, count)
 * pairs (:1100-1122).  THE RESULT IS THEREFORE PINNED TO libstdc++'s std::unordered_map (its bucket counts, its rehash points, its
 * insertion at the front of the element list): built against another standard library the call still follows the cited lines, but
 * tests/golden/branch_reduce.json — its recorded iteration order for keys 0..40 first — would have to be recorded again from a
 * reference built with that library.
 * What is large does not depend on order and runs on the DEVICE.  countUniqueEvidence's filter (:1053-1096) pops, per round, every front
 * equal to the minimum and keeps it only where exactly one list had it; the lists ascend without repeats, so the count of an edge is the
 * number of its ids that occur in NO OTHER LIST OF THE SAME COMPONENT: one stable radix sort of component | id over the ids of all
 * component edges, a comparison with both neighbours, a sum per edge.
 *
 * As the reference has it:
 *  - a branch whose nb_count is 0 is no branch here (:762, :773); a component that holds a false branch is not listed: all its edges are
 *    removed (:849-855, :928-932);
 *  - len1 / len2 of :815-816 / :910-911 are Read::get_len() of the record's read1 / read2 (both mates of a paired read), the record is
 *    getEdgeInfo's: the first outnode -> node in target order;
 *  - every kept neighbour of a skipped component appends the component once more (:172-177: continue, not break); the list is sorted
 *    and de-duplicated afterwards (:206-207), so this shows in no result;
 *  - the diploid rule sorts its pairs with std::sort by count alone (:1104): for four entries that is an insertion sort, ties stay in
 *    the map's iteration order; :1164 compares pairs.at(0) - pairs.at(1), the two SMALLEST counts, with 0.5 * min_evidence;
 *  - countUniqueEvidence consumes evidence_per_edge (pop_front, :1088), so a later component would find the list of a shared edge
 *    empty.  No edge lies in two listed components: a branch is in one component, and the walk that reaches the branch at one end of an
 *    edge goes on to the branch at the other end (the trailing out-branches of :882 are those no in-branch lists).  The call looks for
 *    such an edge all the same (one sort of the component edges, on the host in the walk; of the marks only the no-row one is a kernel's) and would finish its components on the host from the lists themselves;
 *  - a component edge without a key in evidence_per_edge (:1029-1031, also unreachable from hc_br_evidence's tables) shortens
 *    evidence_status, so that index k of it no longer belongs to edge k.  Where the reference then calls at() on the missing key, front()
 *    on an empty list or max_element on an empty vector, the call returns HC_ERR_ARG; otherwise it goes on as the reference does.
 * OverlapGraph::removeEdge (src/OverlapGraph.cpp:104-147) erases the FIRST record u -> v in list order — the graph is in target order,
 * so the first of the run of equal targets — and the FIRST entry u of adj_in[v] in adj_in's own order; edges_to_remove holds a pair
 * once, so of a repeated (u, v) exactly one record leaves and its twins stay.  adj_in keeps its order otherwise.  checkEdge's assert on
 * the score (:242) is not restated. */

typedef struct hc_br_threshold {
    int32_t dist;         /* field 1 of a line of evidence_threshold_table.tsv */
    int32_t min_evidence; /* field 3                                           */
} hc_br_threshold; /* 8 bytes */

typedef struct hc_br_reduce_settings {
    uint32_t careful; /* program_settings.careful                                                                      */
    uint32_t diploid; /* program_settings.diploid                                                                      */
    uint32_t verbose; /* 0: reserved (the reference's prints are not made)                                             */
    uint32_t reserved;
    const hc_br_threshold* thresholds; /* evidence_threshold_map (:134-155); a later entry for the same dist wins       */
    uint64_t n_thresholds;             /* 0: HC_ERR_ARG, the exit(1) of :157                                            */
} hc_br_reduce_settings; /* 32 bytes */

/* What became of a listed component in the chain of :163-204. */
enum {
    HC_BR_RED_KEPT = 0,         /* countUniqueEvidence returned true: the component is in components_kept           */
    HC_BR_RED_NOT_KEPT = 1,     /* it returned false                                                                */
    HC_BR_RED_NO_THRESHOLD = 2, /* evidence_threshold_map has no entry for dist: all edges removed (:193-201)       */
    HC_BR_RED_CAREFUL = 3       /* a neighbouring component was kept earlier: all edges removed (:172-177)          */
};
/* Why the host finished a component (bits; 0: the device's counts and its general rule decided it). */
enum { HC_BR_RED_HOST_NO_ROW = 1, HC_BR_RED_HOST_SHARED_EDGE = 2, HC_BR_RED_HOST_DIPLOID = 4 };

typedef struct hc_br_component {
    int32_t dist;
    int32_t min_evidence;   /* -1: no threshold entry, or not looked up (HC_BR_RED_CAREFUL)                          */
    uint32_t outcome;       /* HC_BR_RED_*                                                                           */
    uint32_t host_finished; /* HC_BR_RED_HOST_* bits; the mirror sets the same bits for the same components         */
    uint64_t edge_first;    /* comp_edge[edge_first, edge_first + edge_count): sorted, unique (:837-847)             */
    uint32_t edge_count;
    uint32_t pad;           /* 0 */
} hc_br_component; /* 32 bytes */

typedef struct hc_br_reduce_counts {
    uint64_t n_components;       /* branching_components                                                              */
    uint64_t n_component_edges;  /* their edges                                                                       */
    uint64_t n_false_dropped;    /* components dropped for a false branch (:849-855, :928-932)                        */
    uint64_t n_no_threshold;     /* HC_BR_RED_NO_THRESHOLD                                                            */
    uint64_t n_careful_dropped;  /* HC_BR_RED_CAREFUL                                                                 */
    uint64_t n_kept;             /* HC_BR_RED_KEPT                                                                    */
    uint64_t n_removed;          /* edges_to_remove after :206-207 = records that left the graph                      */
    uint64_t n_missing_appended; /* missing_edges appended to branching_edges (:83-85)                                */
    uint64_t n_items_sorted;     /* evidence ids of all component edges (device call: the radix sort's items)         */
    uint64_t n_host_finished;    /* components with host_finished != 0                                                */
    double ms_device;            /* device call only: kernels, sort, sums and the edit by events                      */
    double ms_host_walk;         /* device call only: the component walk and the chain, by the host's clock           */
    double ms_copy;              /* device call only: waiting for the copies between host and device                  */
    double ms_sort;              /* device call only: the radix sort's share of ms_device                             */
    double ms_edit;              /* device call only: the edit's share of ms_device (the pairs' records, compaction)   */
} hc_br_reduce_counts; /* 120 bytes */

/* Count, then fetch: every pointer may be NULL (not wanted); a wanted table whose cap is below its count: HC_ERR_ARG, nothing copied.
 *   components   in branching_components order
 *   comp_edge    pairs u, v (2 * cap_comp_edges entries), component by component
 *   comp_unique  per comp_edge entry its unique-evidence count (unique_evidence_per_edge's list length); 0 for a component
 *                countUniqueEvidence was not called for (HC_BR_RED_NO_THRESHOLD, HC_BR_RED_CAREFUL)
 *   removed      edges_to_remove after sort and unique, pairs u, v (2 * cap_removed entries) */
typedef struct hc_br_reduce_tables {
    hc_br_component* components;
    uint64_t cap_components;
    uint32_t* comp_edge;
    uint32_t* comp_unique;
    uint64_t cap_comp_edges;
    uint32_t* removed;
    uint64_t cap_removed;
} hc_br_reduce_tables; /* 56 bytes */

/* The file loop of :137-155 on the bytes of an evidence_threshold_table.tsv: lines end at '\n' (getline); an empty line or one that
 * starts with '#' is skipped; fields are split at tabs, field 1 is dist and field 3 min_evidence, each read as std::stoi reads it
 * (leading white space, a sign, digits; what follows the digits is ignored); a later line for the same dist wins.  out: room for cap
 * entries, in ascending dist; *n is always the number of distinct dists (count, then fetch: HC_ERR_ARG with nothing copied where cap is
 * too small or out is NULL).  A line std::stoi would throw on — no digits, a missing third field, a value outside int —: HC_ERR_ARG and
 * *bad_line = its 1-based number.  bad_line may be NULL. */
int hc_host_br_parse_thresholds(const char* text, uint64_t len, hc_br_threshold* out, uint64_t cap, uint64_t* n, uint64_t* bad_line);

/* HC_ERR_STATE unless the tables of the last hc_br_evidence are still valid (hc_br_evidence_fetch's conditions) and the store it read is
 * still the context's.  HC_ERR_ARG: a null argument, an empty threshold table, tables the reference would end on (above).
 * In order: missing_edges are appended to the device's branching_edges (:83-85); the components, the unique evidence, the decisions;
 * edges_to_remove sorted and de-duplicated (:206-207); those records leave the device graph and are appended to branching_edges in that
 * (u, v) order (:217-225).  The graph stays in the target order hc_br_evidence left it in, and hc_graph_fetch,
 * hc_graph_fetch_branching_edges, hc_graph_write_text, hc_graph_merge_pairs, hc_sr_clique_merge and hc_fno1_run work on it as they do
 * after hc_graph_remove_branches.  The evidence tables are spent afterwards: a second hc_br_reduce or an hc_br_evidence_fetch returns
 * HC_ERR_STATE; hc_br_reduce_fetch serves until the next hc_br_evidence, hc_graph_load / hc_graph_resolve, hc_set_reads or hc_reset.
 * A pair of edges_to_remove without a record in the graph (the exit(1) of :219-222, :1252-1257; unreachable from hc_br_evidence's
 * tables): HC_ERR_ARG, the graph and branching_edges untouched, the tables spent.
 * A fixed number of launches whatever the degrees and list sizes: a lane per final_branch neighbour for (len1, len2,
 * overlap len0) of its record; the host's walk; a lane per component edge for its row of ev_edge (bisection) and its list length, one
 * exclusive sum, a lane per evidence item for the key component << id bits | id (only the bits in use are sorted), one stable radix
 * sort, a lane per sorted item against both neighbours, one exclusive sum and a lane per edge for its count, a lane per component for
 * the general rule of :1243-1271; the host's chain; a wave per removed pair for its record (bisection) and its adj_in entry (the first
 * match by ballot), then the compaction hc_graph_remove_branches uses. */
int hc_br_reduce(hc_ctx* ctx, const hc_br_reduce_settings* settings, hc_br_reduce_counts* counts);
/* The tables of the last hc_br_reduce (cap_* in the struct).  HC_ERR_STATE: none kept. */
int hc_br_reduce_fetch(hc_ctx* ctx, hc_br_reduce_tables* tables);

/* The same on the host (no device, no context): the mirror and the yardstick, the reference statement by statement on one thread.
 * in: the graph and the store as hc_host_br_evidence takes them (adj_out in any order: the mirror sorts a copy as sortAdjOut does; the
 * dict and the original reads are not read); ev: tables as hc_br_evidence_fetch / hc_host_br_evidence fill them, cap_* = their counts.
 * counts is always filled.  tables and graph may be NULL; count, then fetch — or one call with room for the upper bounds: components <=
 * branches, component edges and removed pairs <= branch_nb entries, edges <= the graph's, branching <= missing + the graph's edges. */
typedef struct hc_br_host_graph_out {
    hc_edge_rec* edges;   /* the reduced graph in target order                        */
    uint64_t cap_edges;
    uint64_t* out_off;    /* n_vertices + 1                                           */
    uint32_t* in_nodes;   /* room for cap_edges                                       */
    uint64_t* in_off;     /* n_vertices + 1                                           */
    hc_edge_rec* branching; /* what the call appends to branching_edges, in order     */
    uint64_t cap_branching;
    uint64_t n_edges, n_branching; /* always filled                                   */
} hc_br_host_graph_out; /* 72 bytes */
int hc_host_br_reduce(const hc_br_host_input* in, const hc_br_tables* ev, const hc_br_reduce_settings* settings, hc_br_reduce_counts* counts,
                      hc_br_reduce_tables* tables, hc_br_host_graph_out* graph);
/* std::unordered_map< node_id_t, bool > filled with keys 0 .. n - 1 ascending: its iteration order into order (room for n).  What the
 * host's walk depends on, for tests that pin it. */
int hc_host_br_map_order(uint64_t n, uint64_t* order);

/* ---- singles.fastq, paired1.fastq, paired2.fastq and removed_tip_sequences.fastq from the device ----------------------------
 *
 * The last writer family of SRBuilder (src/SRBuilder.cpp:1386-1556): every iteration ends by appending its reads to singles.fastq,
 * paired1.fastq and paired2.fastq — the last iteration's singles.fastq IS the assembler's result — and the tips it removed to
 * removed_tip_sequences.fastq.  hc_sr_fastq_write_text writes the four texts on the device from raw arrays the context keeps,
 * without a base or quality byte crossing the link before the text itself does.
 *
 * Files 0 - 2 are the context's CURRENT store: whatever hc_set_reads, hc_sr_set_next_reads, hc_sr_merge_next or hc_sr_clique_next last
 * loaded while hc_sr_keep_device was on.  Read r, in ascending r: a single-end read puts "@r\nSEQ\n+\nQUAL\n" into singles.fastq, a
 * paired one "@r\nSEQ1\n+\nQUAL1\n" into paired1.fastq and the same with mate 2 into paired2.fastq; r in decimal, the bytes as stored.
 * That IS the reference's files: the next store numbers the single-end super-reads from 0, then the trivial ones in vertex order, then
 * the paired ones (:1142, :1231-1233, :1280, :1377-1378), and writeSinglesToFile, writeTrivialsToFile and writePairsToFile run in that
 * order, each appending its reads in ascending id (:1484-1487, :1434-1447, :1528-1535) — so every file holds its reads in ascending id
 * of the store, which is the order here.
 * The reference opens its files in append mode; here a text is ONE iteration's contribution, and the caller appends or truncates.
 *
 * File 3 (writeTipsToFile, :1386-1414): tip k — new_ID = k, from 0 in every call — is read vertex_read[tips[k]], taken FORWARD whatever
 * the vertex's orientation: tips_vec.push_back(*read) (:1302, :1309) copies the stored read.  A paired read writes
 * "@k_1\nSEQ1\n+\nQ1\n@k_2\nSEQ2\n+\nQ2\n", a single-end one "@k\nSEQ\n+\nQ\n".  tips / vertex_read are hc_sr_merge_next_output.tips and
 * hc_sr_merge_next_input.vertex_read as they are; n_tips = 0 with NULL pointers is allowed.
 * The tips are reads of the store the last next-store call READ, not of the one it left: after a replacement that store's raw arrays
 * are still on the device (the call trades blocks), and the context remembers it; after HC_SR_NEXT_EMPTY, or when no such call ran
 * since hc_set_reads, it is the current store.  A later next-store call moves on: tips are then reads of the store THAT call read.
 *
 * HC_ERR_STATE: keeping is off, or no kept raw arrays.  HC_ERR_ARG: a tip vertex >= n_vertices, a vertex_read of a tip that is no read
 * of that store (both found by a host pass over the tips before any launch), 2^32 tips or more.  An error leaves the kept text as it
 * was.  The text stays in the context until the next hc_sr_fastq_write_text or until raw arrays it was made from are replaced
 * (hc_set_reads, a next-store call that replaces the store, hc_sr_keep_device(ctx, 0), hc_reset); a fetch after that: HC_ERR_STATE.
 * Four launches whatever the sizes: a lane per read and per tip for the records' characters, one exclusive sum that lays the four files
 * behind one another, the boundaries, and a wave per record that copies sequence and quality with 16-byte stores on 16-byte boundaries
 * of the text.  All sizes and offsets are 64-bit: a file may exceed 4 GiB.
 * Left to the caller: the files themselves — opening, appending or truncating, compression. */

enum { HC_SR_FASTQ_SINGLES = 0, HC_SR_FASTQ_PAIRED1 = 1, HC_SR_FASTQ_PAIRED2 = 2, HC_SR_FASTQ_TIPS = 3 };

typedef struct hc_sr_fastq_counts {
    uint64_t n_records[4]; /* '@' lines per file */
    uint64_t n_bytes[4];   /* characters per file */
    double ms_device;      /* this section's kernels and sums, by events on the context's stream */
} hc_sr_fastq_counts;      /* 72 bytes */

int hc_sr_fastq_write_text(hc_ctx* ctx, const uint32_t* tips, uint64_t n_tips, const uint32_t* vertex_read, uint64_t n_vertices,
                           hc_sr_fastq_counts* counts);

/* Copies bytes [first, first + count) of file HC_SR_FASTQ_* out.  A range outside the file, or file > 3: HC_ERR_ARG; count = 0 is OK,
 * also for an empty file; no text: HC_ERR_STATE. */
int hc_sr_fastq_text_fetch(hc_ctx* ctx, uint32_t file, uint64_t first, uint64_t count, char* dst);

/* The same texts on the host (no device, no context) from a store as hc_set_reads takes it.  file: 0, 1 or 2.  text: room for cap bytes;
 * *n_bytes is always filled, and where cap is too small or text is NULL nothing is copied and HC_ERR_ARG is returned (count, then fetch).
 * HC_ERR_ARG also: a null array, a read that owns neither 1 nor 2 sequences, descending offsets. */
int hc_host_sr_fastq_text(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                          uint32_t n_reads, uint32_t file /* 0..2 */, char* text, uint64_t cap, uint64_t* n_bytes);
/* writeTipsToFile (:1386-1414) for the reads tip_reads[k] of the store, k = new_ID: the caller maps vertices to reads itself.  A tip
 * read >= n_reads: HC_ERR_ARG.  cap / *n_bytes as above (count, then fetch). */
int hc_host_sr_fastq_tips_text(const uint8_t* bases, const uint8_t* quals, const uint64_t* seq_off, const uint32_t* read_first_seq,
                               uint32_t n_reads, const uint32_t* tip_reads, uint64_t n_tips, char* text, uint64_t cap, uint64_t* n_bytes);

/* ---- FNO=1 from the context's graph: SRBuilder::findNextOverlaps on the device ------------------------------------------------
 *
 * Every edge-merge iteration ends with findNextOverlaps (src/FindNextOverlaps.cpp:890-958).  hc_fno1_run (include/hcfno.h) takes host
 * arrays; hc_fno1_from_graph reads what the context holds where it is: adj_out (the graph's records and offsets), branching_edges
 * (hc_graph_remove_tips / hc_graph_remove_branches), the inclusion groups (hc_graph_remove_inclusions) and, with HC_FNO1_TABLES_KEPT, the
 * vertex and super-read tables the last hc_sr_merge_next / hc_sr_clique_next built.  Only the stored non-edges (nonedge_overlaps.txt) and,
 * with HC_FNO1_TABLES_CALLER, the tables come from the host, one upload each.
 *
 * The result is what hc_fno1_run writes for the same facts: the same bytes of overlaps.txt and the same four counters.  adj_out is taken
 * in the list order the graph has AT THE MOMENT OF THE CALL, vertex by vertex, each list front to back, as the reference walks it at
 * :612; a caller that wants the lists in sortEdges' order sorts them first (hc_graph_sort_edges).
 *
 * The edge list updateOverlap is called on is, in this order,
 *   1. adj_out vertex by vertex (:612-624),
 *   2. branching_edges (:627-630),
 *   3. the stored non-edges that pass :694 — checkEdge(v1, v2, true) > 0 drops a line; left out with HC_FNO_OPTIMIZE (:926),
 *   4. the inclusion-induced edges (:816-887): per group every pair i < j in (group, i, j) order, the case analysis of :841-865, no
 *      paired read, len and perc of :870-871, kept where checkEdge(node1, node2, true) == -1 — a record of score 0 IS an edge here.
 * checkEdge answers with the first match in list order, v's list before w's (src/OverlapGraph.cpp:233-259).
 * counts gives the four lengths; hc_fno1_edges_fetch returns the list, and hc_host_fno1_walk_edges builds the same list on the host
 * from an hc_fno1_input, so that the two can be compared array by array.  Feeding the list to hc_fno1_run as plain graph_edges (no
 * other source) reproduces the text.
 *
 * tables = HC_FNO1_TABLES_CALLER: nodes .. subreads are host arrays as in hc_fno1_input (n_nodes must be the graph's vertex count,
 * the super-reads single-end first: anything else is HC_ERR_ARG).  HC_FNO1_TABLES_KEPT: the tables stay where hc_sr_merge_next /
 * hc_sr_clique_next built them; the context remembers them from a successful call of either (HC_OK) until the start of the next one or
 * hc_reset.  In both forms the subread maps are ordered on the device, by one stable radix sort of super-read << 32 | node.
 *
 * Statuses.  HC_ERR_ARG: a NULL argument, HC_FNO_ADD_DUPLICATES (the workflows never set it with this route: hc_fno1_run remains the
 * route for it), a flag bit nobody defined, an unknown `tables`, max_induced_pairs above 2^31 - 16.  HC_ERR_STATE: no valid graph;
 * HC_FNO1_TABLES_KEPT with no tables, or with tables for another vertex count than the graph's.  HC_ERR_NOT_ON_DEVICE: an input the
 * device does not decide — something the reference would stop at (an assert, an .at()), an id >= 10^10 or ids that need more than 31
 * bits, a perc > 999, a count >= 2^31 - 16, more pairs (i, j) than max_induced_pairs; the call then changes nothing, and the caller takes
 * hc_graph_fetch + hc_fno1_run, which reports what the reference reports.  No line at all is HC_OK with n_lines = 0.
 *
 * The text, the edge list and the lines stay in the context until the next hc_fno1_from_graph or the next call that replaces or edits
 * the graph or replaces the store (hc_graph_load, hc_graph_resolve, the cleaning calls, hc_set_reads, hc_reset); a fetch after that:
 * HC_ERR_STATE.  hc_fno1_text_fetch / hc_fno1_edges_fetch: count, then fetch; ranges are 64-bit, a range outside is HC_ERR_ARG.
 * hc_fno1_lines_device: the lines of the text as hc_line_rec in DEVICE memory, in file order — what hc_textblock_submit_lines takes —
 * with the text's columns: perc2 = 0, pos1 / pos2 as the 32 bits of the int the text prints.
 *
 * On the device: a lane per 80-byte record writes one hc_fno_edge with 16-byte loads and stores; a lane per pair (i < j) of a group,
 * found by bisection in one exclusive sum of l (l - 1) / 2, the pair from the triangular index in integer arithmetic; checkEdge by a
 * lane for lists of fewer than 64 records, by a wave, 64 records at a time, for longer ones; survivors placed by ordered selection; the
 * walk, the four stable radix sorts and the text are hc_fno1_run's own launches.  A fixed number of launches, all on the context's
 * stream, grow-only memory, no atomics on the outputs. */
#define HC_FNO1_TABLES_CALLER 0u /* the eight table fields below are host arrays, as in hc_fno1_input */
#define HC_FNO1_TABLES_KEPT   1u /* the tables the last hc_sr_merge_next / hc_sr_clique_next left on the device; the eight fields and new_read_count are ignored */
typedef struct hc_fno1_resident_input {
    uint32_t tables, flags;            /* HC_FNO1_TABLES_*; HC_FNO_RESOLVE_ORIENTATIONS | HC_FNO_NO_INCLUSIONS | HC_FNO_OPTIMIZE */
    const hc_fno_read* nodes;  uint64_t n_nodes;
    const hc_fno_read* srs;    uint64_t n_srs;
    const uint64_t* clique_off; const uint64_t* clique_nodes;
    const uint64_t* subread_off; const hc_fno_subread* subreads;   /* any order inside a super-read */
    const hc_fno_edge* nonedges; uint64_t n_nonedges;              /* host; nonedge_overlaps.txt as today; may be NULL */
    uint64_t new_read_count;
    double edge_threshold;
    uint64_t max_induced_pairs;        /* 0: 2^31 - 16 */
} hc_fno1_resident_input; /* 112 bytes */
typedef struct hc_fno1_resident_counts {
    uint64_t n_lines, n_bytes, copied, u2sr, v2sr, sr2sr;          /* hc_fno_counters' */
    uint64_t n_graph_edges, n_branching, n_nonedges_kept, n_induced_pairs, n_induced, n_items;
    double ms_device;                                              /* events on the context's stream: the sum of hc_fno1_section_ms' four parts */
} hc_fno1_resident_counts; /* 104 bytes */
int hc_fno1_from_graph(hc_ctx* ctx, const hc_fno1_resident_input* in, hc_fno1_resident_counts* counts);
int hc_fno1_text_fetch(hc_ctx* ctx, uint64_t first, uint64_t n_bytes, char* dst);            /* count, then fetch; 64-bit ranges */
int hc_fno1_edges_fetch(hc_ctx* ctx, uint64_t first, uint64_t n, hc_fno_edge* dst);          /* the walk's edge list, see above */
int hc_fno1_lines_device(hc_ctx* ctx, const hc_line_rec** d_lines, uint64_t* n_lines);       /* what hc_textblock_submit_lines takes */
/* The parts of the last call's counts.ms_device, each one event pair on the context's stream: ms[0] the groups' pair counts and their sum;
 * ms[1] the two conversions, checkEdge for the non-edges and the pairs with their selections, the tables' check and the subread maps'
 * sort; ms[2] segments 3 and 4; ms[3] the walk, the sorts, the text and the lines.  ms[3] spans hc_fno1_run's own launch sequence, which
 * waits for the host several times (counts come back between its launches): it is the stream's elapsed time including those gaps, not
 * the kernels' time alone.  A part the call did not reach is 0. */
int hc_fno1_section_ms(hc_ctx* ctx, double ms[4]);
/* The walk's edge list on the host (no device, no context) from an hc_fno1_input, as host/FindNextOverlaps.cpp builds it: n_seg = the
 * four lengths, always filled; out has room for cap records, and where cap is too small or out is NULL nothing is copied and HC_ERR_ARG is
 * returned (count, then fetch).  HC_ERR_FORMAT where the reference would stop, HC_ERR_ARG for HC_FNO_ADD_DUPLICATES. */
int hc_host_fno1_walk_edges(const hc_fno1_input* in, hc_fno_edge* out, uint64_t cap, uint64_t n_seg[4]);  /* host, no device */

#ifdef __cplusplus
}
#endif
#endif
