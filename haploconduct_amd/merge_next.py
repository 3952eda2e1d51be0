"""The rest of SRBuilder::mergeAlongEdges in one call (include/hcsr.h: hc_sr_merge_next and the host mirror hc_host_sr_merge_next): the
survivors of process_cliques with the self-overlap test (reference src/SRBuilder.cpp:981-1001), the `visited` marks (:1260-1277), the
trivial super-reads and the tips list (:1282-1373), the numbering, the next store and the vertex / super-read tables of find-next-overlaps.
Structures, result type and the plumbing shared by EdgeScorer.sr_merge_next (device) and host.sr_merge_next (the mirror)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .consensus import SR_LAYOUT_DTYPE, SR_MEMBER_DTYPE, SR_SUBREAD_DTYPE
from .fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE
from .next_reads import NEXT_EMPTY
from .readstore import ReadSet

MN_NONE, MN_DROPPED_EMPTY, MN_DROPPED_N_RATE, MN_SINGLE, MN_SINGLE_SELF, MN_PAIRED = range(6)                # HC_SR_MN_*
MN_V_MERGED, MN_V_TRIVIAL, MN_V_SHORT, MN_V_N_RATE, MN_V_INCLUSION, MN_V_TIP, MN_V_BAD = range(7)             # HC_SR_MN_V_*

_vp = C.c_void_p


class hc_sr_merge_next_input(C.Structure):
    _fields_ = [("pairs", _vp), ("n_pairs", C.c_uint64), ("pair_status", _vp), ("first_layout", _vp), ("layouts", _vp), ("members", _vp),
                ("n_members", C.c_uint64), ("status", _vp), ("out_off", _vp), ("subreads", _vp), ("vertex_read", _vp), ("vertex_fwd", _vp),
                ("n_vertices", C.c_uint64), ("inclusions", _vp), ("tip_reads", _vp)]


class hc_sr_merge_next_settings(C.Structure):
    _fields_ = [("keep_singletons", C.c_uint32), ("ignore_inclusions", C.c_uint32), ("store_tips_separately", C.c_uint32),
                ("no_self_overlap", C.c_uint32), ("self", N.hc_sr_self_settings)]


class hc_sr_merge_next_output(C.Structure):
    _fields_ = [(k, _vp) for k in ("pair_kind", "pair_new_id", "overlap_pos", "self_score", "vertex_state", "nodes", "srs", "sr_pair", "clique_off",
                                   "clique_nodes", "subread_off", "subreads", "tips")] + \
               [(k, C.c_uint64) for k in ("n_srs", "n_singles", "n_trivials", "n_paired", "n_tips", "n_self_merged", "new_read_count")] + \
               [("counts", N.hc_sr_next_counts), ("self_stats", N.hc_sr_self_stats), ("ms_device", C.c_double), ("ms_copy", C.c_double)]


N.lib.hc_sr_merge_next.restype = C.c_int
N.lib.hc_sr_merge_next.argtypes = [_vp, C.POINTER(hc_sr_merge_next_input), C.POINTER(hc_sr_merge_next_settings), C.POINTER(hc_sr_merge_next_output)]
N.lib.hc_host_sr_merge_next.restype = C.c_int
N.lib.hc_host_sr_merge_next.argtypes = [C.POINTER(N.hc_settings), _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint64, C.POINTER(hc_sr_merge_next_input),
                                        C.POINTER(hc_sr_merge_next_settings), C.POINTER(hc_sr_merge_next_output), _vp, _vp, C.c_uint64,
                                        C.POINTER(C.c_uint64), _vp, _vp]

ARRAYS = ("pair_kind", "pair_new_id", "overlap_pos", "self_score", "vertex_state", "nodes", "srs", "sr_pair", "clique_off", "clique_nodes",
          "subread_off", "subreads", "tips")


@dataclass
class MergeNext:
    pair_kind: np.ndarray     # uint32 per pair: MN_*
    pair_new_id: np.ndarray   # int32 per pair
    overlap_pos: np.ndarray   # int32 per pair
    self_score: np.ndarray    # float64 per pair
    vertex_state: np.ndarray  # uint32 per vertex: MN_V_*
    nodes: np.ndarray         # FNO_READ_DTYPE per vertex
    srs: np.ndarray           # FNO_READ_DTYPE per surviving super-read, singles then pairs
    sr_pair: np.ndarray       # uint32: the pair behind each
    clique_off: np.ndarray
    clique_nodes: np.ndarray
    subread_off: np.ndarray
    subreads: np.ndarray      # FNO_SUBREAD_DTYPE, two per super-read
    tips: np.ndarray          # uint32: the vertices of tips_vec
    n_singles: int
    n_trivials: int
    n_paired: int
    n_self_merged: int
    new_read_count: int
    counts: dict              # hc_sr_next_counts
    self_stats: dict
    ms_device: float
    ms_copy: float
    empty: bool               # nothing survived: the old store is in place (device) / reads is None (mirror)
    reads: ReadSet = None     # the mirror: the arrays one would pass to set_reads next

    def fno1_input(self, graph_edges, **kw):
        """fno.input_from_merge_next(self, graph_edges, **kw)"""
        from . import fno

        return fno.input_from_merge_next(self, graph_edges, **kw)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _prepare(pairs, edge, vertex_read, vertex_fwd, inclusions, tip_reads, keep_singletons, ignore_inclusions, store_tips_separately, self_overlap,
             min_score, min_qual, min_overlap, n_threads):
    """edge: a consensus.SrEdgeLayouts with .result (what EdgeScorer.sr_edge_merge returned)."""
    pairs = _c(pairs, np.uint32).reshape(-1, 2)
    n = pairs.shape[0]
    a = dict(pairs=pairs, pair_status=_c(edge.pair_status, np.uint32), first_layout=_c(edge.first_layout, np.uint64), layouts=_c(edge.layouts, SR_LAYOUT_DTYPE),
             members=_c(edge.members, SR_MEMBER_DTYPE), status=_c(edge.result.status, np.uint32), out_off=_c(edge.result.out_off, np.uint64),
             subreads=_c(edge.subreads, SR_SUBREAD_DTYPE).reshape(-1), vertex_read=_c(vertex_read, np.uint32), vertex_fwd=_c(vertex_fwd, np.uint8),
             inclusions=None if inclusions is None else _c(inclusions, np.uint8), tip_reads=None if tip_reads is None else _c(tip_reads, np.uint8))
    nv = a["vertex_read"].size
    if a["pair_status"].size != n or a["first_layout"].size != n + 1 or a["subreads"].size != 2 * n or a["vertex_fwd"].size != nv:
        raise ValueError("the per-pair / per-vertex arrays differ in length")
    nl = int(a["first_layout"][-1]) if n else 0
    if a["layouts"].size < nl or a["status"].size < nl or a["out_off"].size < nl + 1:
        raise ValueError("fewer layouts than first_layout names")
    if a["inclusions"] is not None and a["inclusions"].size != nv:
        raise ValueError("inclusions has not one byte per vertex")
    inp = hc_sr_merge_next_input()
    for k, v in a.items():
        setattr(inp, k, _ptr(v))
    inp.n_pairs, inp.n_members, inp.n_vertices = n, a["members"].size, nv
    st = hc_sr_merge_next_settings(int(keep_singletons), int(bool(ignore_inclusions)), int(bool(store_tips_separately)), int(not self_overlap),
                                   N.hc_sr_self_settings(float(min_score), float(min_qual), int(min_overlap), int(n_threads)))
    o = dict(pair_kind=np.zeros(n, np.uint32), pair_new_id=np.full(n, -1, np.int32), overlap_pos=np.full(n, -1, np.int32), self_score=np.zeros(n),
             vertex_state=np.zeros(nv, np.uint32), nodes=np.zeros(nv, FNO_READ_DTYPE), srs=np.zeros(n, FNO_READ_DTYPE), sr_pair=np.zeros(n, np.uint32),
             clique_off=np.zeros(n + 1, np.uint64), clique_nodes=np.zeros(4 * n, np.uint64), subread_off=np.zeros(n + 1, np.uint64),
             subreads=np.zeros(2 * n, FNO_SUBREAD_DTYPE), tips=np.zeros(nv, np.uint32))
    out = hc_sr_merge_next_output()
    for k, v in o.items():
        setattr(out, k, v.ctypes.data)  # (an empty numpy array still has an address)
    return a, inp, st, o, out


def _result(o, out, empty, reads=None):
    ns, nc = int(out.n_srs), int(o["clique_off"][int(out.n_srs)])
    return MergeNext(o["pair_kind"], o["pair_new_id"], o["overlap_pos"], o["self_score"], o["vertex_state"], o["nodes"], o["srs"][:ns], o["sr_pair"][:ns],
                     o["clique_off"][:ns + 1], o["clique_nodes"][:nc], o["subread_off"][:ns + 1], o["subreads"][:2 * ns], o["tips"][:int(out.n_tips)],
                     int(out.n_singles), int(out.n_trivials), int(out.n_paired), int(out.n_self_merged), int(out.new_read_count), out.counts.as_dict(),
                     {k: getattr(out.self_stats, k) for k, _ in out.self_stats._fields_}, float(out.ms_device), float(out.ms_copy), empty, reads)


def merge_next(ctx, pairs, edge, vertex_read, vertex_fwd, inclusions=None, tip_reads=None, keep_singletons=0, ignore_inclusions=False,
               store_tips_separately=False, self_overlap=True, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=16, n_reads=None):
    """hc_sr_merge_next on a context (EdgeScorer.sr_merge_next).  n_reads: the reads of the context's store, where the caller knows them —
    tip_reads is then checked to hold a byte for each (the call reads that many)."""
    keep, inp, st, o, out = _prepare(pairs, edge, vertex_read, vertex_fwd, inclusions, tip_reads, keep_singletons, ignore_inclusions,
                                     store_tips_separately, self_overlap, min_score, min_qual, min_overlap, n_threads)
    if n_reads is not None and keep["tip_reads"] is not None and keep["tip_reads"].size < n_reads:
        raise ValueError("tip_reads has not one byte per read of the store")
    rc = N.lib.hc_sr_merge_next(ctx, C.byref(inp), C.byref(st), C.byref(out))
    if rc not in (0, NEXT_EMPTY):
        N.check(rc, "hc_sr_merge_next")
    return _result(o, out, rc == NEXT_EMPTY)


def host_merge_next(reads, cons_seq, cons_qual, pairs, edge, vertex_read, vertex_fwd, settings=None, inclusions=None, tip_reads=None, keep_singletons=0,
                    ignore_inclusions=False, store_tips_separately=False, self_overlap=True, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=1):
    """hc_host_sr_merge_next: the host mirror.  reads: the current ReadSet; cons_seq / cons_qual: the kept consensus bytes; settings: a
    records.Settings, of which --mismatch and --min_read_len are read (the self-overlap test)."""
    from .records import Settings

    keep, inp, st, o, out = _prepare(pairs, edge, vertex_read, vertex_fwd, inclusions, tip_reads, keep_singletons, ignore_inclusions,
                                     store_tips_separately, self_overlap, min_score, min_qual, min_overlap, n_threads)
    cs = (settings or Settings()).to_c()
    cons_seq, cons_qual = _c(cons_seq, np.uint8), _c(cons_qual, np.uint8)
    if cons_seq.size != cons_qual.size:
        raise ValueError("cons_seq and cons_qual differ in length")
    if keep["tip_reads"] is not None and keep["tip_reads"].size < reads.n_reads:
        raise ValueError("tip_reads has not one byte per read of the store")
    n = int(inp.n_pairs + inp.n_vertices)
    off, first = np.zeros(2 * n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    nb = C.c_uint64()

    def once(ob, oq, cap):
        return N.lib.hc_host_sr_merge_next(C.byref(cs), _ptr(reads.bases), _ptr(reads.quals), reads.seq_off.ctypes.data, reads.read_first_seq.ctypes.data,
                                           reads.n_reads, _ptr(cons_seq), _ptr(cons_qual), cons_seq.size, C.byref(inp), C.byref(st), C.byref(out), _ptr(ob),
                                           _ptr(oq), cap, C.byref(nb), off.ctypes.data, first.ctypes.data)

    rc = once(None, None, 0)  # count ...
    if rc == NEXT_EMPTY:
        return _result(o, out, True)
    if rc != 0 and out.counts.n_kept == 0:
        N.check(rc, "hc_host_sr_merge_next")
    ob, oq = np.zeros(nb.value, np.uint8), np.zeros(nb.value, np.uint8)
    N.check(once(ob, oq, ob.size), "hc_host_sr_merge_next")  # ... then fetch
    nr, ns = int(out.counts.n_kept), int(out.counts.n_seq)
    return _result(o, out, False, ReadSet(ob, oq, off[:ns + 1], first[:nr + 1], np.arange(nr, dtype=np.uint64)))
