"""EdgeScorer — Python face of the hc_ctx C-ABI (include/hcedge.h).

It plays the role of the reference's ``EdgeCalculator`` object for the scoring half
of the path (reference src/EdgeCalculator.h:25-64): constructed from the settings,
given the reads once, then fed batches of candidate overlaps."""
import ctypes as C

import numpy as np

from . import _native as N
from .records import ADMIT_DTYPE, CAND_DTYPE, OVERLAP_DTYPE, REC_COMPACT, REC_FULL, RESULT_DTYPE, ROW_DTYPE, TEXT_NONPLAIN_DTYPE, TEXT_REJECT_DTYPE, TEXT_ROW_DTYPE, Settings


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


class EdgeScorer:
    def __init__(self, settings: Settings = None):
        self.settings = settings or Settings()
        self._cs = self.settings.to_c()
        self._ctx = C.c_void_p()
        N.check(N.lib.hc_create(C.byref(self._ctx), C.byref(self._cs)), "hc_create")
        self._reads = None

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            N.lib.hc_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def reset(self, settings):
        """hc_reset: the context takes new settings and is as after its creation (no reads: call set_reads again); its device memory stays."""
        cs = settings.to_c()
        N.check(N.lib.hc_reset(self._ctx, C.byref(cs)), "hc_reset")
        self.settings, self._cs, self._reads = settings, cs, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- reads --------------------------------------------------------------
    def set_reads(self, reads):
        self._reads = reads
        N.check(
            N.lib.hc_set_reads(self._ctx, _ptr(reads.bases), _ptr(reads.quals), _ptr(reads.seq_off),
                               _ptr(reads.read_first_seq), reads.n_reads),
            "hc_set_reads",
        )

    def set_reads_from_fastq(self, singles=None, paired1=None, paired2=None, ids=None, max_reads=0):
        """hc_set_reads_from_fastq_text: the FASTQ files (paths or bytes; ids: the --IDs file's path) read on the device into the store, as
        host.Fastq followed by set_reads would leave it.  Returns the fastq_reader.hc_fastq_counts; the ids and offsets: fastq_fetch."""
        from . import fastq_reader as FR

        cn = FR.set_reads_from_fastq(self._ctx, singles, paired1, paired2, ids, max_reads)
        self._reads, self._fastq_counts = None, cn  # (the reads live on the device)
        return cn

    def fastq_fetch(self):
        """hc_fastq_fetch: (read_ids, seq_off, read_first_seq) of the store the last set_reads_from_fastq read."""
        from . import fastq_reader as FR

        cn = getattr(self, "_fastq_counts", None)
        return FR.fetch(self._ctx, cn if cn is not None else FR.hc_fastq_counts())

    def fastq_set_chunk_bytes(self, n_bytes):
        """hc_fastq_set_chunk_bytes: a test switch — the upload's chunk (0: the default)."""
        from . import fastq_reader as FR

        FR.set_chunk_bytes(self._ctx, n_bytes)

    # -- super-read consensus (include/hcsr.h) --------------------------------
    def sr_consensus(self, layouts, members, min_qual=0.99, min_clique_size=2, error_correction=False, subreads_needed=False, n_threads=16):
        """hc_sr_consensus: SRBuilder::consensus (src/SRBuilder.cpp:413-535) for every layout, on the device against the store of
        set_reads.  layouts / members: consensus.SR_LAYOUT_DTYPE / SR_MEMBER_DTYPE records.  Returns a consensus.SrResult."""
        from . import consensus as SR

        st = SR.make_settings(min_qual, min_clique_size, error_correction, subreads_needed, n_threads)
        return SR.run(lambda *a: N.lib.hc_sr_consensus(self._ctx, *a), layouts, members, st)

    def sr_merge_self_overlaps(self, seq, qual, pairs, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=16, count_first=False):
        """hc_sr_merge_self_overlaps: SRBuilder::merge_self_overlap (src/SRBuilder.cpp:872-955) for every pair, on the device.  seq / qual:
        packed bytes (what sr_consensus returns as cons_seq / cons_qual), pairs: consensus.SR_PAIR_DTYPE records.  --mismatch and
        --min_read_len are this scorer's settings.  Needs no set_reads.  Returns a consensus.SrSelfResult."""
        from . import consensus as SR

        st = SR.make_self_settings(min_score, min_qual, min_overlap, n_threads)
        return SR.run_self(lambda *a: N.lib.hc_sr_merge_self_overlaps(self._ctx, *a), seq, qual, pairs, st, count_first)

    def sr_merge_self_overlaps_kept(self, pairs, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=16):
        """hc_sr_merge_self_overlaps_kept: the same merge with the mates read from the consensus bytes kept on the device (sr_keep_device,
        then sr_consensus / sr_edge_merge / sr_kept_load) and the merged reads appended to them.  pairs index the kept bytes.  Returns a
        consensus.SrSelfKeptResult: out_off holds absolute kept offsets, which sr_set_next_reads takes as SR_SRC_CONSENSUS."""
        from . import consensus as SR

        return SR.run_self_kept(self._ctx, pairs, SR.make_self_settings(min_score, min_qual, min_overlap, n_threads))

    def sr_kept_load(self, seq, qual):
        """hc_sr_kept_load: packed bytes of the caller's become the kept consensus bytes."""
        from . import consensus as SR

        SR.kept_load(self._ctx, seq, qual)

    def sr_kept_fetch(self, off=0, n=None):
        """hc_sr_kept_fetch: (seq, qual) = bytes [off, off + n) of the kept consensus bytes (n = None: to their end)."""
        from . import consensus as SR

        return SR.kept_fetch(self._ctx, off, n)

    # -- edge merges on the device graph (include/hcsr.h) -----------------------
    def graph_merge_pairs(self, with_stats=False):
        """hc_graph_merge_pairs: OverlapGraph::getEdgesForMerging (src/GraphAlgos.cpp:112-148) on the device graph; (n, 2) vertex ids in
        the order taken (with_stats: and the hc_merge_pairs_stats as a dict)."""
        from . import consensus as SR

        st = N.hc_merge_pairs_stats()
        V, _ = self._graph_size()
        pairs = SR.merge_pairs(lambda p, cap, n: N.lib.hc_graph_merge_pairs(self._ctx, p, cap, n, C.byref(st)), V)
        return (pairs, {k: getattr(st, k) for k, _ in st._fields_}) if with_stats else pairs

    def sr_edge_merge(self, pairs, vertex_read, vertex_fwd, min_qual=0.99, min_clique_size=2, error_correction=False, subreads_needed=False,
                      n_threads=16, cap=None):
        """hc_sr_edge_merge: SRBuilder::mergeAlongEdges' layouts (sort_vertices, src/SRBuilder.cpp:33-285), consensus and calcSubreadInfo
        (:536-595) for pairs of vertices of the device graph.  Returns a consensus.SrEdgeLayouts with .result (a consensus.SrResult)."""
        from . import consensus as SR

        st = SR.make_settings(min_qual, min_clique_size, error_correction, subreads_needed, n_threads)
        return SR.edge_merge(self._ctx, pairs, vertex_read, vertex_fwd, st, cap)

    def sr_clique_merge(self, clique_off, clique_nodes, vertex_read, vertex_fwd, min_qual=0.99, min_clique_size=2, error_correction=False,
                        subreads_needed=False, n_threads=16, cap=None):
        """hc_sr_clique_merge: constructSuperread (src/SRBuilder.cpp:654-748) for cliques of any size of the device graph, given as a CSR of
        vertex ids — sort_vertices, filter_subreads, consensus and calcSubreadInfo.  Returns a consensus.SrCliqueLayouts with .result."""
        from . import consensus as SR

        st = SR.make_settings(min_qual, min_clique_size, error_correction, subreads_needed, n_threads)
        return SR.clique_merge(self._ctx, clique_off, clique_nodes, vertex_read, vertex_fwd, st, cap)

    def sr_clique_filter_on_host(self, on=True):
        """hc_sr_clique_filter_on_host: a test switch — every filtered layout of sr_clique_merge goes to the host's filter."""
        N.check(N.lib.hc_sr_clique_filter_on_host(self._ctx, 1 if on else 0), "sr_clique_filter_on_host")

    # -- the next iteration's store from super-reads (include/hcsr.h) -----------
    def sr_keep_device(self, on=True):
        """hc_sr_keep_device: set_reads keeps its raw arrays and sr_consensus its output on the device (off by default)."""
        N.check(N.lib.hc_sr_keep_device(self._ctx, int(bool(on))), "hc_sr_keep_device")

    def sr_set_next_reads(self, entries, extra_seq=None, extra_qual=None, keep_singletons=0):
        """hc_sr_set_next_reads: filter, number and gather the entries (next_reads.NEXT_ENTRY_DTYPE) on the device and replace the store
        by the survivors.  Returns a next_reads.NextReads (empty = True: nothing was kept, the old store is in place)."""
        from . import next_reads as NR

        res = NR.set_next_reads(self._ctx, entries, extra_seq, extra_qual, keep_singletons)
        if not res.empty:
            self._reads = None  # (the new reads live on the device: sr_next_reads_fetch)
        return res

    def sr_next_reads_fetch(self):
        """hc_sr_next_reads_fetch: the kept raw arrays of the current store as a ReadSet."""
        from . import next_reads as NR

        return NR.fetch(self._ctx)

    def sr_merge_next(self, pairs, edge, vertex_read, vertex_fwd, inclusions=None, tip_reads=None, keep_singletons=0, ignore_inclusions=False,
                      store_tips_separately=False, self_overlap=True, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=16):
        """hc_sr_merge_next: the rest of SRBuilder::mergeAlongEdges (src/SRBuilder.cpp:981-1001, 1260-1380) from what sr_edge_merge returned
        (edge: its consensus.SrEdgeLayouts) — the self-overlap test, the `visited` marks, the trivial super-reads, the tips list, the
        numbering, the next store and the vertex / super-read tables of find-next-overlaps.  Returns a merge_next.MergeNext (empty = True:
        nothing survived, the old store is in place)."""
        from . import merge_next as MN

        res = MN.merge_next(self._ctx, pairs, edge, vertex_read, vertex_fwd, inclusions, tip_reads, keep_singletons, ignore_inclusions,
                            store_tips_separately, self_overlap, min_score, min_qual, min_overlap, n_threads,
                            n_reads=self._reads.n_reads if self._reads is not None else None)
        if not res.empty:
            self._reads = None  # (the new reads live on the device: sr_next_reads_fetch)
        return res

    def sr_clique_next(self, clique_off, clique_nodes, merged, vertex_read, vertex_fwd, keep_singletons=0, self_overlap=True, min_score=0.99,
                       min_qual=0.99, min_overlap=15, n_threads=16):
        """hc_sr_clique_next: the rest of SRBuilder::cliquesToSuperreads (src/SRBuilder.cpp:981-1001, 1122-1233) from what sr_clique_merge
        returned (merged: its consensus.SrCliqueLayouts) — the self-overlap test, the `visited` marks, the trivial super-reads, the
        numbering, the next store and the vertex / super-read tables of find-next-overlaps.  Returns a clique_next.CliqueNext (empty = True:
        nothing survived, the old store is in place)."""
        from . import clique_next as CN

        res = CN.clique_next(self._ctx, clique_off, clique_nodes, merged, vertex_read, vertex_fwd, keep_singletons, self_overlap, min_score, min_qual,
                             min_overlap, n_threads)
        if not res.empty:
            self._reads = None  # (the new reads live on the device: sr_next_reads_fetch)
        return res

    def sr_originals_init(self):
        """hc_sr_originals_init: the first iteration's dict of the current store (OverlapGraph::buildOriginalsDict with first_it,
        src/OverlapGraph.cpp:772-797), kept on the device."""
        from . import originals as OR

        OR.init(self._ctx)

    def sr_originals_load(self, off, entries):
        """hc_sr_originals_load: the caller's dict (a CSR over the current store's reads, originals.ORIGINAL_DTYPE entries in ascending id
        inside a read) becomes the kept one."""
        from . import originals as OR

        OR.load(self._ctx, off, entries)

    def sr_originals_fetch(self):
        """hc_sr_originals_fetch: (off, entries) of the kept dict."""
        from . import originals as OR

        return OR.fetch(self._ctx)

    def sr_originals_next(self, res, merged, vertex_read, vertex_fwd, first_it=False):
        """hc_sr_originals_next: the dict of the next store from the kept one and what sr_merge_next / sr_clique_next returned (res) for
        the layouts of sr_edge_merge / sr_clique_merge (merged) — constructSuperread's loop over the originals (src/SRBuilder.cpp:750-806),
        merge_self_overlap's shift (:938-949) and the trivials (:1161-1216, :1312-1369).  res may be an originals.Tables instead (merged is
        then not read).  Returns an originals.OriginalsNext; the new dict replaces the kept one."""
        from . import originals as OR

        t = res if isinstance(res, OR.Tables) else OR.tables_from(res, merged, vertex_read, vertex_fwd, first_it)
        return OR.next_dict(self._ctx, t)

    def sr_originals_text(self):
        """hc_sr_originals_write_text + hc_sr_originals_text_fetch: the bytes of subreads.txt for the kept dict (src/SRBuilder.cpp:1449-1463),
        line k = read k, entries in ascending original id."""
        from . import originals as OR

        return OR.text(self._ctx)[0]

    def fno3_from_originals(self, counts3, original_readcount, walk_rank=None, max_combos=0, flags=0):
        """hc_fno3_from_originals + the fetch of the whole text and candidate table: findNextOverlaps3 (src/FindNextOverlaps3.cpp:20-173) from
        the kept dict and the store's read descriptors.  counts3 = (n_single, n_trivial, n_paired) of the store in id order.  Lines come in
        ascending (walk rank of SR1, walk rank of SR2); a pair that shares several originals is deduced from the one of smallest id, and is
        flagged ambiguous where they disagree (include/hcsr.h).  Returns an originals.Fno3Resident."""
        from . import originals as OR

        return OR.fno3_from_originals(self._ctx, counts3, original_readcount, walk_rank, max_combos, flags)

    def fno1_from_graph(self, tables=None, nonedges=None, edge_threshold=0.97, flags=1, max_induced_pairs=0):
        """hc_fno1_from_graph: findNextOverlaps (src/FindNextOverlaps.cpp:890-958) from the graph, the branching edges and the inclusion
        groups the context holds.  tables: None = the tables the last sr_merge_next / sr_clique_next left on the device; a MergeNext /
        CliqueNext or the tuple (nodes, srs, clique_off, clique_nodes, subread_off, subreads, new_read_count) = host tables.  nonedges:
        fno.FNO_EDGE_DTYPE records of nonedge_overlaps.txt.  Returns a fno.Fno1Resident (counts); the text, the edge list and the lines stay
        on the device: fno1_text, fno1_edges, fno1_lines_device."""
        from . import fno as F

        self._fno1 = F.fno1_from_graph(self._ctx, tables, nonedges, edge_threshold, flags, max_induced_pairs)
        return self._fno1

    def fno1_text(self, piece_bytes=None):
        """hc_fno1_text_fetch: the whole text of the last fno1_from_graph (piece_bytes: fetched in pieces of that many bytes)."""
        from . import fno as F

        n = int(self._fno1.counts["n_bytes"])
        step = int(piece_bytes) if piece_bytes else max(n, 1)
        return b"".join(F.fno1_text(self._ctx, at, min(step, n - at)) for at in range(0, n, step))

    def fno1_edges(self):
        """hc_fno1_edges_fetch: the edge list the last fno1_from_graph walked and its four segment lengths
        ([adj_out][branching_edges][stored non-edges kept][inclusion-induced edges])."""
        from . import fno as F

        c = self._fno1.counts
        seg = [int(c[k]) for k in ("n_graph_edges", "n_branching", "n_nonedges_kept", "n_induced")]
        return F.fno1_edges(self._ctx, 0, sum(seg)), seg

    def fno1_lines_device(self):
        """hc_fno1_lines_device: (device pointer, number) of the last fno1_from_graph's lines as hc_line_rec (records.LINE_DTYPE), what
        hc_textblock_submit_lines takes; found_lines_fetch copies them out."""
        p, n = C.c_void_p(), C.c_uint64()
        N.check(N.lib.hc_fno1_lines_device(self._ctx, C.byref(p), C.byref(n)), "hc_fno1_lines_device")
        return p.value, int(n.value)

    def fno1_section_ms(self):
        """hc_fno1_section_ms: the four parts of the last fno1_from_graph's ms_device — [pair counts, conversions + checkEdge + subread sort,
        segments 3 and 4, the walk with its sorts, text and lines (host waits between its launches included)]."""
        ms = (C.c_double * 4)()
        N.check(N.lib.hc_fno1_section_ms(self._ctx, C.byref(ms)), "hc_fno1_section_ms")
        return [float(x) for x in ms]

    def found_lines_fetch(self, d_lines, n):
        """hc_found_lines_fetch: n hc_line_rec from device memory (records.LINE_DTYPE)."""
        from .records import LINE_DTYPE

        out = np.zeros(int(n), dtype=LINE_DTYPE)
        if n:
            N.check(N.lib.hc_found_lines_fetch(self._ctx, C.c_void_p(d_lines), int(n), _ptr(out)), "hc_found_lines_fetch")
        return out

    def score_lines_device(self, d_lines, n_lines, first_line_no=0):
        """hc_textblock_submit_lines + hc_textblock_wait: parsed lines in device memory through a text block of their own, as score_text
        takes the text.  Returns the block's dict (the hc_text_result fields, rows / rejected as numpy copies)."""
        b = C.c_void_p()
        N.check(N.lib.hc_textblock_create(self._ctx, max(64 * int(n_lines), 4096), C.byref(b)), "hc_textblock_create")
        try:
            if int(N.lib.hc_textblock_max_lines(b)) < n_lines:
                raise ValueError("more lines than a text block takes")
            N.check(N.lib.hc_textblock_submit_lines(b, C.c_void_p(d_lines), int(n_lines), int(first_line_no), 0), "hc_textblock_submit_lines")
            r = N.hc_text_result()
            N.check(N.lib.hc_textblock_wait(b, C.byref(r)), "hc_textblock_wait")
            return self._text_result(b, r, 0)
        finally:
            N.lib.hc_textblock_destroy(b)

    def br_set_original_reads(self, bases, seq_off):
        """hc_br_set_original_reads: the sequences of --original_fastq (single-end, one byte per base, n + 1 offsets), kept on the device."""
        from . import branch_evidence as BR

        BR.set_original_reads(self._ctx, bases, seq_off)

    def br_evidence(self, vertex_read, vertex_fwd, settings):
        """hc_br_evidence: findBranchingEvidence (src/BranchReduction.cpp:229-743) for every branch of the device graph, from the kept store,
        the kept dict and the original reads.  settings: branch_evidence.settings(...).  Leaves adj_out in target order.  Returns the counts
        (a dict, "some_failed" among them); br_evidence_fetch returns the tables."""
        from . import branch_evidence as BR

        d, self._br_counts = BR.evidence(self._ctx, vertex_read, vertex_fwd, settings)
        return d

    def br_evidence_fetch(self):
        """hc_br_evidence_fetch: the tables of the last br_evidence as a branch_evidence.BranchEvidence."""
        from . import branch_evidence as BR

        cn = getattr(self, "_br_counts", None)
        return BR.fetch(self._ctx, cn if cn is not None else BR.hc_br_counts())

    def br_reduce(self, settings):
        """hc_br_reduce: the second half of readBasedBranchReduction (src/BranchReduction.cpp:82-227, :745-1272) on the tables of the last
        br_evidence: the device graph loses edges_to_remove, branching_edges gains the missing edges and the removed records.  settings:
        branch_evidence.reduce_settings(...).  Returns the counts (a dict); br_reduce_fetch returns the tables."""
        from . import branch_evidence as BR

        d, self._br_reduce_counts = BR.reduce(self._ctx, settings)
        return d

    def br_reduce_fetch(self):
        """hc_br_reduce_fetch: the tables of the last br_reduce as a branch_evidence.BranchReduction."""
        from . import branch_evidence as BR

        cn = getattr(self, "_br_reduce_counts", None)
        return BR.reduce_fetch(self._ctx, cn if cn is not None else N.hc_br_reduce_counts())

    def sr_fastq_text(self, tips=None, vertex_read=None):
        """hc_sr_fastq_write_text + hc_sr_fastq_text_fetch: the bytes of singles.fastq, paired1.fastq and paired2.fastq for the current store
        and of removed_tip_sequences.fastq for the tips of the last sr_merge_next (its .tips and the vertex_read it took), as written by
        src/SRBuilder.cpp:1386-1556.  Returns a dict: "singles", "paired1", "paired2", "tips" (bytes), "n_records", "n_bytes" (per file, in
        that order), "ms_device"."""
        from . import fastq_text as FQ

        return FQ.text(self._ctx, tips, vertex_read)

    def info(self):
        k, sb = C.c_uint32(), C.c_uint64()
        d = [C.c_double() for _ in range(4)]
        N.check(N.lib.hc_get_info(self._ctx, C.byref(k), C.byref(sb), *[C.byref(x) for x in d]), "hc_get_info")
        return {"qual_alphabet": k.value, "store_bytes": sb.value, "x_edge": (d[0].value, d[1].value),
                "x_ov": (d[2].value, d[3].value)}

    def kernel_info(self, n=0):
        """hc_get_kernel_info[_for]: the scoring kernel chosen for the read set (n > 0: for a launch of n candidates), as text."""
        buf = C.create_string_buffer(768)
        N.check(N.lib.hc_get_kernel_info_for(self._ctx, int(n), buf, 768), "hc_get_kernel_info_for")
        return buf.value.decode()

    def locality_order(self):
        """hc_get_locality_order: the reads in the order a launch scores their runs in (an empty array: no order for this read set)."""
        n = C.c_uint64()
        N.check(N.lib.hc_get_locality_order(self._ctx, None, 0, C.byref(n)), "hc_get_locality_order")
        out = np.empty(n.value, np.uint32)
        N.check(N.lib.hc_get_locality_order(self._ctx, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), "hc_get_locality_order")
        return out

    def set_reorder(self, mode):
        """0 never, 1 always, 2 auto (hc_set_reorder)."""
        N.check(N.lib.hc_set_reorder(self._ctx, int(mode)), "hc_set_reorder")

    # -- scoring ------------------------------------------------------------
    def score_batch(self, overlaps):
        """Host buffers in, host buffers out (hc_score_batch)."""
        ov = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        out = np.empty(ov.shape[0], dtype=RESULT_DTYPE)
        N.check(N.lib.hc_score_batch(self._ctx, _ptr(ov), ov.shape[0], _ptr(out)), "hc_score_batch")
        return out

    @staticmethod
    def pack_cands(overlaps):
        """hc_pack_cands: hc_overlap_rec -> hc_cand_rec (16 bytes: what the device reads)."""
        ov = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        out = np.empty(ov.shape[0], dtype=CAND_DTYPE)
        N.lib.hc_pack_cands(_ptr(ov), ov.shape[0], _ptr(out))
        return out

    def score_cands(self, cands):
        """Compact records in, result records out (hc_score_cands; host buffers)."""
        cd = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        out = np.empty(cd.shape[0], dtype=RESULT_DTYPE)
        N.check(N.lib.hc_score_cands(self._ctx, _ptr(cd), cd.shape[0], _ptr(out)), "hc_score_cands")
        return out

    def score_cands_device(self, d_in_ptr, n, d_out_ptr, stream=None):
        N.check(N.lib.hc_score_cands_device(self._ctx, C.c_void_p(d_in_ptr), n, C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)),
                "hc_score_cands_device")

    def score_blocks(self, cands, block=250000, in_flight=2):
        """The stage's device leg on a whole candidate array: hc_block_submit / hc_block_wait over blocks of `block`
        compact records, `in_flight` block objects; returns the non-dropped rows of all blocks in index order."""
        cd = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        n = cd.shape[0]
        blocks = []
        for _ in range(in_flight):
            b = C.c_void_p()
            N.check(N.lib.hc_block_create(self._ctx, max(1, min(block, max(n, 1))), C.byref(b)), "hc_block_create")
            blocks.append(b)
        out, pending = [], []

        def wait(b):
            rows, k = C.c_void_p(), C.c_uint64()
            N.check(N.lib.hc_block_wait(b, C.byref(rows), C.byref(k)), "hc_block_wait")
            if k.value:
                out.append(np.frombuffer((C.c_char * (k.value * 32)).from_address(rows.value), dtype=ROW_DTYPE).copy())

        try:
            for i, at in enumerate(range(0, n, block)):
                b = blocks[i % in_flight]
                if len(pending) == in_flight:
                    wait(pending.pop(0))
                m = min(block, n - at)
                N.check(N.lib.hc_block_submit(b, C.c_void_p(cd.ctypes.data + at * 16), m, at), "hc_block_submit")
                pending.append(b)
            while pending:
                wait(pending.pop(0))
        finally:
            for b in blocks:
                N.lib.hc_block_destroy(b)
        return np.concatenate(out) if out else np.zeros(0, ROW_DTYPE)

    def set_ids(self, read_ids):
        """hc_text_set_ids: the id -> read index table of the device's text parser."""
        ids = np.ascontiguousarray(read_ids, dtype=np.uint64)
        N.check(N.lib.hc_text_set_ids(self._ctx, _ptr(ids), ids.shape[0]), "hc_text_set_ids")

    def score_text(self, text, block_bytes=1 << 20, first_line_no=0, chained=False, reserve_rows=0, list_nonplain=0, max_bytes=None):
        """The overlaps file's TEXT through hc_textblock_submit / hc_textblock_wait, block by block (cut at line ends; an empty text is
        one empty block).  Returns a list with one dict per block: the hc_text_result fields, rows / rejected as numpy copies.
        chained: hc_textblock_submit_from — the text goes to the device straight from `text`, two blocks in flight, line
        numbers through an hc_linechain (first_line_no must be 0).  reserve_rows: hc_textblock_reserve_rows before the first submit;
        every dict carries "regrown" = hc_textblock_regrown of the block so far.  list_nonplain: hc_textblock_list_nonplain with that
        many entries before the first submit (True: hc_textblock_max_lines of them); every dict then carries "nonplain", a copy of the
        listed lines (TEXT_NONPLAIN_DTYPE), and "max_lines".  max_bytes: the size the blocks are created with (None: block_bytes)."""
        raw = text if isinstance(text, bytes) else text.encode()
        max_bytes = max(block_bytes if max_bytes is None else max_bytes, 64)
        if chained:
            return self._score_text_chained(raw, block_bytes, list_nonplain, max_bytes)
        b = C.c_void_p()
        N.check(N.lib.hc_textblock_create(self._ctx, max_bytes, C.byref(b)), "hc_textblock_create")
        out, at, line_no, base = [], 0, first_line_no, 0
        try:
            if reserve_rows:
                N.check(N.lib.hc_textblock_reserve_rows(b, reserve_rows), "hc_textblock_reserve_rows")
            self._list_nonplain(b, list_nonplain)
            buf = N.lib.hc_textblock_buffer(b)
            while at < len(raw) or not out:
                end = min(len(raw), at + block_bytes)
                if end < len(raw):
                    nl = raw.rfind(b"\n", at, end)
                    if nl < 0:
                        raise ValueError("a line longer than the block")
                    end = nl + 1
                C.memmove(buf, raw[at:end], end - at)
                N.check(N.lib.hc_textblock_submit(b, end - at, line_no, base), "hc_textblock_submit")
                r = N.hc_text_result()
                N.check(N.lib.hc_textblock_wait(b, C.byref(r)), "hc_textblock_wait")
                d = self._text_result(b, r, list_nonplain)
                d["base"], d["bytes"] = base, (at, end)
                d["regrown"] = int(N.lib.hc_textblock_regrown(b))
                out.append(d)
                line_no += r.n_lines
                base += r.n_lines
                at = end
        finally:
            N.lib.hc_textblock_destroy(b)
        return out

    @staticmethod
    def _list_nonplain(b, list_nonplain):
        if list_nonplain:
            n = int(N.lib.hc_textblock_max_lines(b)) if list_nonplain is True else int(list_nonplain)
            N.check(N.lib.hc_textblock_list_nonplain(b, n), "hc_textblock_list_nonplain")

    @staticmethod
    def _text_result(b, r, list_nonplain):
        d = {k: getattr(r, k) for k, _ in r._fields_ if k not in ("rows", "rejected", "nonplain")}
        d["rows"] = np.frombuffer((C.c_char * (r.n_rows * 80)).from_address(r.rows), dtype=TEXT_ROW_DTYPE).copy() if r.n_rows else np.zeros(0, TEXT_ROW_DTYPE)
        d["rejected"] = (np.frombuffer((C.c_char * (r.n_rejected * 56)).from_address(r.rejected), dtype=TEXT_REJECT_DTYPE).copy()
                         if r.n_rejected else np.zeros(0, TEXT_REJECT_DTYPE))
        if list_nonplain:
            d["nonplain"] = (np.frombuffer((C.c_char * (r.n_nonplain_listed * 16)).from_address(r.nonplain), dtype=TEXT_NONPLAIN_DTYPE).copy()
                             if r.n_nonplain_listed else np.zeros(0, TEXT_NONPLAIN_DTYPE))
            d["max_lines"] = int(N.lib.hc_textblock_max_lines(b))
        return d

    def _score_text_chained(self, raw, block_bytes, list_nonplain, max_bytes):
        cuts, at = [], 0
        while at < len(raw) or not cuts:
            end = min(len(raw), at + block_bytes)
            if end < len(raw):
                nl = raw.rfind(b"\n", at, end)
                if nl < 0:
                    raise ValueError("a line longer than the block")
                end = nl + 1
            cuts.append((at, end))
            at = end
        src = np.frombuffer(raw, np.uint8)  # pageable host memory, read in place
        blocks = [C.c_void_p(), C.c_void_p()]
        chain = C.c_void_p()
        for b in blocks:
            N.check(N.lib.hc_textblock_create(self._ctx, max_bytes, C.byref(b)), "hc_textblock_create")
            self._list_nonplain(b, list_nonplain)
        N.check(N.lib.hc_linechain_create(self._ctx, len(cuts), C.byref(chain)), "hc_linechain_create")
        out, base = [], 0

        def collect(k):
            nonlocal base
            r = N.hc_text_result()
            N.check(N.lib.hc_textblock_wait(blocks[k % 2], C.byref(r)), "hc_textblock_wait")
            d = self._text_result(blocks[k % 2], r, list_nonplain)
            d["base"], d["bytes"] = base, cuts[k]
            base += r.n_lines
            out.append(d)

        try:
            for k, (a, e) in enumerate(cuts):
                if k >= 2:
                    collect(k - 2)
                N.check(N.lib.hc_textblock_submit_from(blocks[k % 2], (src.ctypes.data + a) if e > a else None, e - a, chain, k,
                                                       blocks[(k - 1) % 2] if k else None, 0),
                        "hc_textblock_submit_from")
            for k in range(max(0, len(cuts) - 2), len(cuts)):
                collect(k)
        finally:
            for b in blocks:
                N.lib.hc_textblock_destroy(b)
            N.lib.hc_linechain_destroy(chain)
        return out

    def graph_resolve(self, admitted, n_vertices, vertex_of_read=None, sorted_order=False, pieces=0):
        """hc_graph_resolve + hc_graph_fetch: duplicate resolution and adjacency lists on the device.  Returns a dict
        with counts, edges (EDGE_DTYPE), out_off, in_nodes, in_off, seq, inclusions, tied_vertices.
        pieces > 0: hand the records over with hc_graph_begin / hc_graph_append in that many pieces first."""
        from .host import EDGE_DTYPE

        adm = np.ascontiguousarray(admitted, dtype=ADMIT_DTYPE)
        gc = N.hc_graph_counts()
        vtx = None if vertex_of_read is None else np.ascontiguousarray(vertex_of_read, dtype=np.uint32)
        src = _ptr(adm)
        if pieces > 0:
            N.check(N.lib.hc_graph_begin(self._ctx), "hc_graph_begin")
            cuts = [adm.shape[0] * k // pieces for k in range(pieces + 1)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                N.check(N.lib.hc_graph_append(self._ctx, C.c_void_p(adm.ctypes.data + a * 48), b - a), "hc_graph_append")
            src = None
        N.check(N.lib.hc_graph_resolve(self._ctx, src, adm.shape[0], n_vertices, None if vtx is None else _ptr(vtx),
                                       1 if sorted_order else 0, C.byref(gc)), "hc_graph_resolve")
        res = {"counts": {k: getattr(gc, k) for k, _ in gc._fields_}}
        if gc.first_bad >= 0:
            return res
        E = int(gc.n_edges)
        edges = np.zeros(E, EDGE_DTYPE)
        out_off, in_off = np.zeros(n_vertices + 1, np.uint64), np.zeros(n_vertices + 1, np.uint64)
        in_nodes, seq = np.zeros(E, np.uint32), np.zeros(E, np.uint32)
        incl = np.zeros(n_vertices, np.uint8)
        tied = np.zeros(int(gc.n_tied_lists), np.uint32)
        N.check(N.lib.hc_graph_fetch(self._ctx, _ptr(edges), _ptr(out_off), _ptr(in_nodes), _ptr(in_off), _ptr(seq), _ptr(incl),
                                     _ptr(tied) if tied.size else None), "hc_graph_fetch")
        res.update(edges=edges, out_off=out_off, in_nodes=in_nodes, in_off=in_off, seq=seq, inclusions=incl, tied_vertices=tied)
        return res

    def graph_load(self, edges, out_off, in_nodes, in_off, inclusions=None):
        """hc_graph_load: a caller's CSR graph (adj_out records, adj_in) onto the device in place of the resolved one."""
        from .host import EDGE_DTYPE

        e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        oo, io = np.ascontiguousarray(out_off, np.uint64), np.ascontiguousarray(in_off, np.uint64)
        inn = np.ascontiguousarray(in_nodes, np.uint32)
        inc = None if inclusions is None else np.ascontiguousarray(inclusions, np.uint8)
        N.check(N.lib.hc_graph_load(self._ctx, _ptr(e), _ptr(oo), _ptr(inn), _ptr(io), oo.size - 1, e.shape[0],
                                    None if inc is None else _ptr(inc)), "hc_graph_load")

    def graph_label_vertices(self, resolve_orientations=True, add_duplicates=False, n_reads=0):
        """hc_graph_label_vertices: OverlapGraph::vertexLabellingHeuristic + checkDuplicateEdges on the device graph; returns the counts
        (counts["status"]: N.LABEL_STATUS).  The labels: graph_orientations()."""
        st, c = N.label_settings(resolve_orientations, add_duplicates, n_reads), N.hc_label_counts()
        N.check(N.lib.hc_graph_label_vertices(self._ctx, C.byref(st), C.byref(c)), "hc_graph_label_vertices")
        return c.as_dict()

    def graph_orientations(self):
        """hc_graph_fetch_orientations: vertex_orientations of the last graph_label_vertices, one byte per vertex (the vertex_fwd of the
        merge calls)."""
        V, _ = self._graph_size()
        fwd = np.zeros(V, np.uint8)
        N.check(N.lib.hc_graph_fetch_orientations(self._ctx, _ptr(fwd) if V else None, V), "hc_graph_fetch_orientations")
        return fwd

    def graph_remove_inclusions(self):
        """hc_graph_remove_inclusions: OverlapGraph::removeInclusions on the device graph; returns the counts."""
        c = N.hc_clean_counts()
        N.check(N.lib.hc_graph_remove_inclusions(self._ctx, C.byref(c)), "hc_graph_remove_inclusions")
        return c.as_dict()

    def graph_remove_transitive(self, remove_trans, branch_reduction=False):
        """hc_graph_remove_transitive: OverlapGraph::removeTransitiveEdges on the device graph; returns the counts."""
        c = N.hc_clean_counts()
        N.check(N.lib.hc_graph_remove_transitive(self._ctx, remove_trans, 1 if branch_reduction else 0, C.byref(c)),
                "hc_graph_remove_transitive")
        return c.as_dict()

    def graph_inclusion_edges(self):
        """hc_graph_fetch_inclusion_edges: (group vertices, group offsets, records) of the last removeInclusions."""
        from .host import EDGE_DTYPE

        ng, ne = C.c_uint64(), C.c_uint64()
        N.check(N.lib.hc_graph_fetch_inclusion_edges(self._ctx, None, None, None, 0, C.byref(ng), C.byref(ne)), "hc_graph_fetch_inclusion_edges")
        gv, off = np.zeros(ng.value, np.uint32), np.zeros(ng.value + 1, np.uint64)
        out = np.zeros(ne.value, EDGE_DTYPE)
        N.check(N.lib.hc_graph_fetch_inclusion_edges(self._ctx, _ptr(gv) if gv.size else None, _ptr(off), _ptr(out) if out.size else None,
                                                     ne.value, C.byref(ng), C.byref(ne)), "hc_graph_fetch_inclusion_edges")
        return gv, off, out

    def graph_remove_tips(self, max_tip_len, read_geom):
        """hc_graph_remove_tips: OverlapGraph::removeTips on the device graph; read_geom (READ_GEOM_DTYPE) is indexed by
        the records' read1 / read2.  Returns the counts."""
        from .host import READ_GEOM_DTYPE

        rg = np.ascontiguousarray(read_geom, dtype=READ_GEOM_DTYPE)
        c = N.hc_tip_counts()
        N.check(N.lib.hc_graph_remove_tips(self._ctx, max_tip_len, _ptr(rg) if rg.size else None, rg.shape[0], C.byref(c)), "hc_graph_remove_tips")
        return c.as_dict()

    def graph_remove_branches(self):
        """hc_graph_remove_branches: OverlapGraph::removeBranches on the device graph; returns the counts."""
        c = N.hc_branch_counts()
        N.check(N.lib.hc_graph_remove_branches(self._ctx, C.byref(c)), "hc_graph_remove_branches")
        return c.as_dict()

    def graph_branching_edges(self):
        """hc_graph_fetch_branching_edges: what removeTips / removeBranches removed so far, in removal order (EDGE_DTYPE)."""
        from .host import EDGE_DTYPE

        n = C.c_uint64()
        N.check(N.lib.hc_graph_fetch_branching_edges(self._ctx, None, 0, C.byref(n)), "hc_graph_fetch_branching_edges")
        out = np.zeros(n.value, EDGE_DTYPE)
        if out.size:
            N.check(N.lib.hc_graph_fetch_branching_edges(self._ctx, _ptr(out), out.size, C.byref(n)), "hc_graph_fetch_branching_edges")
        return out

    def graph_tip_reads(self, n_reads):
        """hc_graph_fetch_tip_reads: Read::is_tip() of reads [0, n_reads) as bytes."""
        out = np.zeros(n_reads, np.uint8)
        N.check(N.lib.hc_graph_fetch_tip_reads(self._ctx, _ptr(out) if n_reads else None, n_reads), "hc_graph_fetch_tip_reads")
        return out

    def graph_write_text(self, kind, edge_threshold=0.0, merge_contigs=0.0, n_singles=0, piece_bytes=None):
        """hc_graph_write_text + hc_graph_text_fetch: graph.txt ("cliques"), digraph.txt ("digraph") or a GFA file ("gfa") of the device
        graph as (bytes, counts).  piece_bytes: fetch the text in pieces of that many bytes.  A failed reference assert: empty bytes and
        counts["status"] != 0 (N.GRAPH_TEXT_STATUS)."""
        st = N.hc_graph_text_settings(edge_threshold, merge_contigs, n_singles)
        c = N.hc_graph_text_counts()
        N.check(N.lib.hc_graph_write_text(self._ctx, N.GRAPH_TEXT_KINDS.get(kind, kind), C.byref(st), C.byref(c)), "hc_graph_write_text")
        if c.status != 0:
            return b"", c.as_dict()
        out = np.empty(int(c.n_bytes), np.uint8)
        step = int(piece_bytes) if piece_bytes else max(out.size, 1)
        for first in range(0, out.size, step):
            n = min(step, out.size - first)
            N.check(N.lib.hc_graph_text_fetch(self._ctx, first, n, _ptr(out[first:first + n])), "hc_graph_text_fetch")
        return out.tobytes(), c.as_dict()

    def graph_cliques(self, root_cap=0, max_entries=0, n_threads=16, fetch=True):
        """hc_graph_cliques + hc_graph_cliques_fetch: the maximal cliques of the device graph (the graph of graph.txt) as a cliques.Cliques —
        what quick-cliques computes for the reference, in the call's own order.  root_cap: the largest root degree the device takes (0:
        the default), max_entries: the budget (0: 2^31 - 1).  fetch=False leaves the CSR on the device and returns the counts."""
        from . import cliques as CL

        return CL.graph_cliques(self._ctx, root_cap, max_entries, n_threads, fetch)

    def graph_sort_edges(self, len_by_read):
        """hc_graph_sort_edges: OverlapGraph::sortEdges (src/OverlapGraph.cpp:722-764) on the device graph, whatever order it is in;
        len_by_read[r] = total length of read r.  Returns the counts (n_edges, n_tied_lists)."""
        from . import cycles as CY

        return CY.graph_sort_edges(self._ctx, len_by_read)

    def graph_remove_cycles(self, remove_edges=True):
        """hc_graph_remove_cycles + hc_graph_fetch_cycle_pairs: OverlapGraph::cycleRemovalHeuristic on the device graph as hc_graph_sort_edges
        left it.  Returns a cycles.CycleRemoval (pairs = the lines of cycles.txt, counts)."""
        from . import cycles as CY

        return CY.graph_remove_cycles(self._ctx, remove_edges)

    def graph_fetch(self):
        """hc_graph_fetch of the graph the device holds: edges, out_off, in_nodes, in_off, seq, inclusions."""
        from .host import EDGE_DTYPE

        V, E = self._graph_size()
        edges = np.zeros(E, EDGE_DTYPE)
        out_off, in_off = np.zeros(V + 1, np.uint64), np.zeros(V + 1, np.uint64)
        in_nodes, seq, incl = np.zeros(E, np.uint32), np.zeros(E, np.uint32), np.zeros(V, np.uint8)
        N.check(N.lib.hc_graph_fetch(self._ctx, _ptr(edges) if E else None, _ptr(out_off), _ptr(in_nodes) if E else None, _ptr(in_off),
                                     _ptr(seq) if E else None, _ptr(incl) if V else None, None), "hc_graph_fetch")
        return dict(edges=edges, out_off=out_off, in_nodes=in_nodes, in_off=in_off, seq=seq, inclusions=incl)

    def _graph_size(self):
        V, E = C.c_uint64(), C.c_uint64()
        N.check(N.lib.hc_graph_size(self._ctx, C.byref(V), C.byref(E)), "hc_graph_size")
        return int(V.value), int(E.value)

    def score_batch_compact(self, overlaps):
        """hc_score_batch_compact: (indices, records) of the non-DROP candidates only."""
        ov = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        n = ov.shape[0]
        idx = np.empty(n, dtype=np.uint32)
        res = np.empty(n, dtype=RESULT_DTYPE)
        k = C.c_uint64()
        N.check(N.lib.hc_score_batch_compact(self._ctx, _ptr(ov), n, _ptr(idx), _ptr(res), n, C.byref(k)),
                "hc_score_batch_compact")
        return idx[: k.value].copy(), res[: k.value].copy()

    def compact_device(self, d_results_ptr, n, d_indices_ptr, d_count_ptr, stream=None):
        N.check(N.lib.hc_compact_device(self._ctx, C.c_void_p(d_results_ptr), n, C.c_void_p(d_indices_ptr),
                                        C.c_void_p(d_count_ptr), C.c_void_p(stream or 0)), "hc_compact_device")

    def find_overlaps(self, err_rate, min_overlap, reversals=True, inclusions=True, count_only=False):
        """hc_find_overlaps: all suffix-prefix overlaps / inclusions between the stored sequences (SFO records).
        count_only: compute on the device (always afresh) and return the number of records."""
        from .records import FIND_INCLUSIONS, FIND_REVERSALS, SFO_DTYPE

        flags = (FIND_REVERSALS if reversals else 0) | (FIND_INCLUSIONS if inclusions else 0)
        n = C.c_uint64()
        N.check(N.lib.hc_find_overlaps(self._ctx, err_rate, min_overlap, flags | 4, None, 0, C.byref(n)), "hc_find_overlaps")
        if count_only:
            return int(n.value)
        out = np.zeros(n.value, SFO_DTYPE)
        if n.value:
            N.check(N.lib.hc_find_overlaps(self._ctx, err_rate, min_overlap, flags, out.ctypes.data, out.size, C.byref(n)), "hc_find_overlaps")
        return out[: n.value]

    def found_to_overlaps(self, out_path, num_singles, num_pairs):
        """hc_found_to_overlaps: the SFO ingest (scripts/sfo2overlaps.py) straight from the records the last find_overlaps
        left on the device — flip and sort there, matching on the host threads.  Returns the number of overlap lines."""
        n = C.c_uint64()
        N.check(N.lib.hc_found_to_overlaps(self._ctx, str(out_path).encode(), int(num_singles), int(num_pairs), C.byref(n)), "hc_found_to_overlaps")
        return int(n.value)

    def set_found_records(self, recs):
        """hc_set_found_records: SFO records from elsewhere (records.SFO_DTYPE) in the place of the finder's."""
        recs = np.ascontiguousarray(recs)
        N.check(N.lib.hc_set_found_records(self._ctx, _ptr(recs), recs.size), "hc_set_found_records")

    def set_found_from_sfo_text(self, text):
        """hc_set_found_from_sfo_text: the SFO file's text (bytes) read on the device into the finder's place.  Returns the number of records;
        raises HcError (HC_ERR_NOT_ON_DEVICE) for a text that is not canonical."""
        n = C.c_uint64()
        N.check(N.lib.hc_set_found_from_sfo_text(self._ctx, text, len(text), C.byref(n)), "hc_set_found_from_sfo_text")
        return int(n.value)

    def found_to_lines(self, num_singles, num_pairs):
        """hc_found_to_lines_device + hc_found_lines_fetch: the SFO ingest entirely on the device; the overlaps file's lines as records
        (records.LINE_DTYPE), in file order.  Raises RuntimeError("... not on the device ...") where the device cannot decide."""
        from .records import LINE_DTYPE

        p, n = C.c_void_p(), C.c_uint64()
        N.check(N.lib.hc_found_to_lines_device(self._ctx, int(num_singles), int(num_pairs), C.byref(p), C.byref(n)), "hc_found_to_lines_device")
        out = np.zeros(n.value, dtype=LINE_DTYPE)
        N.check(N.lib.hc_found_lines_fetch(self._ctx, p, n.value, _ptr(out)), "hc_found_lines_fetch")
        return out

    def set_sam_records(self, sam):
        """hc_set_sam_records: SAM records (host.SamRecords, or anything with alns / recs / ops / ref_len arrays of records.SAM_*_DTYPE) to
        the device.  Raises HcError (HC_ERR_NOT_ON_DEVICE) for records the device does not decide."""
        from .records import SAM_ALN_DTYPE, SAM_OP_DTYPE, SAM_REC_DTYPE

        alns = np.ascontiguousarray(sam.alns, dtype=SAM_ALN_DTYPE)
        recs = np.ascontiguousarray(sam.recs, dtype=SAM_REC_DTYPE)
        ops = np.ascontiguousarray(sam.ops, dtype=SAM_OP_DTYPE)
        ref_len = np.ascontiguousarray(sam.ref_len, dtype=np.uint64)
        N.check(N.lib.hc_set_sam_records(self._ctx, _ptr(alns), alns.size, _ptr(recs), recs.size, _ptr(ops), ops.size, _ptr(ref_len), ref_len.size),
                "hc_set_sam_records")

    def sam_plan(self, min_overlap_len):
        """hc_sam_plan: the enumeration's plan for one min_overlap_len; returns the number of lines of the whole file."""
        n = C.c_uint64()
        N.check(N.lib.hc_sam_plan(self._ctx, int(min_overlap_len), C.byref(n)), "hc_sam_plan")
        return int(n.value)

    def sam_plan_counts(self):
        """hc_sam_plan_counts: (evaluated pairs, records the waves looked at) of the last plan."""
        c, w = C.c_uint64(), C.c_uint64()
        N.check(N.lib.hc_sam_plan_counts(self._ctx, C.byref(c), C.byref(w)), "hc_sam_plan_counts")
        return int(c.value), int(w.value)

    def sam_lines(self, first_line, n):
        """hc_sam_lines_fetch: lines [first_line, first_line + n) of the planned file as records (records.LINE_DTYPE), in file order."""
        from .records import LINE_DTYPE

        out = np.zeros(int(n), dtype=LINE_DTYPE)
        N.check(N.lib.hc_sam_lines_fetch(self._ctx, int(first_line), int(n), _ptr(out)), "hc_sam_lines_fetch")
        return out

    def score_pack_device(self, d_in_ptr, n, d_out_ptr, cap, base_index, d_payload_ptr, stream=None, fmt=REC_FULL):
        """hc_score_pack_device: scoring + the collection payload in one kernel (rows unordered, count in row 0)."""
        N.check(N.lib.hc_score_pack_device(self._ctx, fmt, C.c_void_p(d_in_ptr), n, C.c_void_p(d_out_ptr), cap, base_index,
                                           C.c_void_p(d_payload_ptr), C.c_void_p(stream or 0)), "hc_score_pack_device")
        return True

    def narrow_payload_device(self, d_payload_ptr, cap, d_payload24_ptr, stream=None):
        """hc_narrow_payload_device: a (cap + 1)-row payload of 32-byte rows -> 24-byte rows (x1, x2, index | mm << 32 | n << 46 | class << 60)."""
        N.check(N.lib.hc_narrow_payload_device(self._ctx, C.c_void_p(d_payload_ptr), cap, C.c_void_p(d_payload24_ptr), C.c_void_p(stream or 0)),
                "hc_narrow_payload_device")

    def set_comm_reserve(self, cus):
        """hc_set_comm_reserve: launches leave `cus` CUs to the kernels of the multi-GPU exchange (0: none)."""
        N.check(N.lib.hc_set_comm_reserve(self._ctx, int(cus)), "hc_set_comm_reserve")

    def comm_gate_device(self, stream, timeout_us=0):
        """hc_comm_gate_device: `stream` continues once the workgroups of the score_pack_device launches enqueued so far have started."""
        N.check(N.lib.hc_comm_gate_device(self._ctx, C.c_void_p(stream or 0), int(timeout_us)), "hc_comm_gate_device")

    def compact_pack_device(self, d_results_ptr, n, d_indices_ptr, d_count_ptr, cap, base_index, d_payload_ptr, stream=None):
        """hc_compact_pack_device: compaction + pack, the count in row 0 of the (cap + 1)-row payload."""
        N.check(N.lib.hc_compact_pack_device(self._ctx, C.c_void_p(d_results_ptr), n, C.c_void_p(d_indices_ptr), C.c_void_p(d_count_ptr),
                                             cap, base_index, C.c_void_p(d_payload_ptr), C.c_void_p(stream or 0)), "hc_compact_pack_device")

    def pack_rows_device(self, d_results_ptr, d_indices_ptr, d_count_ptr, cap, base_index, d_rows_ptr, stream=None):
        """hc_pack_rows_device: compacted records -> 32-byte rows tagged with their global candidate index."""
        N.check(N.lib.hc_pack_rows_device(self._ctx, C.c_void_p(d_results_ptr), C.c_void_p(d_indices_ptr), C.c_void_p(d_count_ptr),
                                          cap, base_index, C.c_void_p(d_rows_ptr), C.c_void_p(stream or 0)), "hc_pack_rows_device")

    def score_batch_device(self, d_in_ptr, n, d_out_ptr, stream=None):
        """Device pointers (ints, e.g. torch tensor .data_ptr()); asynchronous."""
        N.check(N.lib.hc_score_batch_device(self._ctx, C.c_void_p(d_in_ptr), n, C.c_void_p(d_out_ptr),
                                            C.c_void_p(stream or 0)), "hc_score_batch_device")

    def synchronize(self):
        N.check(N.lib.hc_synchronize(self._ctx), "hc_synchronize")

    def time_kernel(self, d_in_ptr, n, d_out_ptr, iters, fmt=REC_FULL):
        ms = C.c_float()
        N.check(N.lib.hc_time_score_kernel(self._ctx, fmt, C.c_void_p(d_in_ptr), n, C.c_void_p(d_out_ptr), iters,
                                           C.byref(ms)), "hc_time_score_kernel")
        return float(ms.value)

    def count_positions_device(self, d_in_ptr, n, fmt=REC_FULL):
        a, b = C.c_uint64(), C.c_uint64()
        N.check(N.lib.hc_count_positions_device(self._ctx, fmt, C.c_void_p(d_in_ptr), n, C.byref(a), C.byref(b)),
                "hc_count_positions_device")
        return int(a.value), int(b.value)

    def finalize(self, results, allow_errors=False):
        """Host libm finalisation -> (score, mismatch_rate, cls) arrays (hc_finalize_batch)."""
        res = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        n = res.shape[0]
        score = np.empty(n, np.float64)
        mrate = np.empty(n, np.float64)
        cls = np.empty(n, np.uint32)
        st = N.lib.hc_finalize_batch(C.byref(self._cs), _ptr(res), n, _ptr(score), _ptr(mrate), _ptr(cls))
        if st != 0 and not (allow_errors and st == -10):
            raise N.HcError(st, "hc_finalize_batch")
        return score, mrate, cls
