"""The rest of SRBuilder::cliquesToSuperreads in one call (include/hcsr.h: hc_sr_clique_next and the host mirror hc_host_sr_clique_next): the
survivors of process_cliques with the self-overlap test (reference src/SRBuilder.cpp:981-1001), the `visited` marks (:1122-1136), the
trivial super-reads (:1145-1222), the numbering, the next store and the vertex / super-read tables of find-next-overlaps — and the gate in
front of process_cliques (:1056-1084, hc_host_sr_clique_select).  Structures, result type and the plumbing shared by
EdgeScorer.sr_clique_next (device) and host.sr_clique_next (the mirror).  The kinds and vertex states are merge_next's MN_* / MN_V_*."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .consensus import SR_LAYOUT_DTYPE, SR_MEMBER_DTYPE, SR_SUBREAD_DTYPE
from .fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE
from .next_reads import NEXT_EMPTY
from .readstore import ReadSet

_vp = C.c_void_p


class hc_sr_clique_next_input(C.Structure):
    _fields_ = [("clique_off", _vp), ("clique_nodes", _vp), ("n_cliques", C.c_uint64), ("clique_status", _vp), ("first_layout", _vp), ("layouts", _vp),
                ("members", _vp), ("member_vertex", _vp), ("n_members", C.c_uint64), ("status", _vp), ("out_off", _vp), ("subreads", _vp),
                ("vertex_read", _vp), ("vertex_fwd", _vp), ("n_vertices", C.c_uint64)]


class hc_sr_clique_next_settings(C.Structure):
    _fields_ = [("keep_singletons", C.c_uint32), ("no_self_overlap", C.c_uint32), ("self", N.hc_sr_self_settings)]


ARRAYS = ("clique_kind", "clique_new_id", "overlap_pos", "self_score", "vertex_state", "nodes", "srs", "sr_clique", "clique_off", "clique_nodes",
          "subread_off", "subreads")


class hc_sr_clique_next_output(C.Structure):
    _fields_ = [(k, _vp) for k in ARRAYS] + \
               [(k, C.c_uint64) for k in ("n_srs", "n_singles", "n_trivials", "n_paired", "n_self_merged", "new_read_count")] + \
               [("counts", N.hc_sr_next_counts), ("self_stats", N.hc_sr_self_stats), ("ms_device", C.c_double), ("ms_copy", C.c_double)]


N.lib.hc_sr_clique_next.restype = C.c_int
N.lib.hc_sr_clique_next.argtypes = [_vp, C.POINTER(hc_sr_clique_next_input), C.POINTER(hc_sr_clique_next_settings), C.POINTER(hc_sr_clique_next_output)]
N.lib.hc_host_sr_clique_next.restype = C.c_int
N.lib.hc_host_sr_clique_next.argtypes = [C.POINTER(N.hc_settings), _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint64, C.POINTER(hc_sr_clique_next_input),
                                         C.POINTER(hc_sr_clique_next_settings), C.POINTER(hc_sr_clique_next_output), _vp, _vp, C.c_uint64,
                                         C.POINTER(C.c_uint64), _vp, _vp]
N.lib.hc_host_sr_clique_select.restype = C.c_int
N.lib.hc_host_sr_clique_select.argtypes = [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]


@dataclass
class CliqueNext:
    clique_kind: np.ndarray    # uint32 per clique: merge_next.MN_*
    clique_new_id: np.ndarray  # int32 per clique
    overlap_pos: np.ndarray    # int32 per clique
    self_score: np.ndarray     # float64 per clique
    vertex_state: np.ndarray   # uint32 per vertex: merge_next.MN_V_*
    nodes: np.ndarray          # FNO_READ_DTYPE per vertex
    srs: np.ndarray            # FNO_READ_DTYPE per surviving super-read, singles then pairs
    sr_clique: np.ndarray      # uint32: the clique behind each
    clique_off: np.ndarray
    clique_nodes: np.ndarray
    subread_off: np.ndarray
    subreads: np.ndarray       # FNO_SUBREAD_DTYPE, one per clique vertex of each super-read
    n_singles: int
    n_trivials: int
    n_paired: int
    n_self_merged: int
    new_read_count: int
    counts: dict               # hc_sr_next_counts
    self_stats: dict
    ms_device: float
    ms_copy: float
    empty: bool                # nothing survived: the old store is in place (device) / reads is None (mirror)
    reads: ReadSet = None      # the mirror: the arrays one would pass to set_reads next

    def row(self, k):
        return self.clique_nodes[int(self.clique_off[k]):int(self.clique_off[k + 1])]

    def fno1_input(self, graph_edges, **kw):
        """fno.input_from_merge_next(self, graph_edges, **kw): the tables have hc_sr_merge_next's form"""
        from . import fno

        return fno.input_from_merge_next(self, graph_edges, **kw)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _prepare(clique_off, clique_nodes, merged, vertex_read, vertex_fwd, keep_singletons, self_overlap, min_score, min_qual, min_overlap, n_threads):
    """merged: a consensus.SrCliqueLayouts with .result (what EdgeScorer.sr_clique_merge returned)."""
    a = dict(clique_off=_c(clique_off, np.uint64), clique_nodes=_c(clique_nodes, np.uint32), clique_status=_c(merged.clique_status, np.uint32),
             first_layout=_c(merged.first_layout, np.uint64), layouts=_c(merged.layouts, SR_LAYOUT_DTYPE), members=_c(merged.members, SR_MEMBER_DTYPE),
             member_vertex=_c(merged.member_vertex, np.uint32), status=_c(merged.result.status, np.uint32), out_off=_c(merged.result.out_off, np.uint64),
             subreads=_c(merged.subreads, SR_SUBREAD_DTYPE).reshape(-1), vertex_read=_c(vertex_read, np.uint32), vertex_fwd=_c(vertex_fwd, np.uint8))
    if a["clique_off"].size == 0:
        a["clique_off"] = np.zeros(1, np.uint64)
    n, nv = a["clique_off"].size - 1, a["vertex_read"].size
    n_items = int(a["clique_off"][-1])
    if a["clique_status"].size != n or a["first_layout"].size != n + 1 or a["vertex_fwd"].size != nv:
        raise ValueError("the per-clique / per-vertex arrays differ in length")
    if a["clique_nodes"].size < n_items or a["subreads"].size < n_items:
        raise ValueError("fewer clique vertices or subread infos than clique_off names")
    nl = int(a["first_layout"][-1]) if n else 0
    if a["layouts"].size < nl or a["status"].size < nl or a["out_off"].size < nl + 1:
        raise ValueError("fewer layouts than first_layout names")
    # the members the layouts name: hc_sr_clique_merge's buffers have room for more than it fills
    nm = int((a["layouts"]["first_member"][:nl].astype(np.uint64) + a["layouts"]["n_members"][:nl]).max()) if nl else 0
    nm = min(nm, a["member_vertex"].size)
    inp = hc_sr_clique_next_input()
    for k, v in a.items():
        setattr(inp, k, _ptr(v))
    inp.clique_off = a["clique_off"].ctypes.data
    inp.n_cliques, inp.n_members, inp.n_vertices = n, nm, nv
    st = hc_sr_clique_next_settings(int(keep_singletons), int(not self_overlap),
                                    N.hc_sr_self_settings(float(min_score), float(min_qual), int(min_overlap), int(n_threads)))
    o = dict(clique_kind=np.zeros(n, np.uint32), clique_new_id=np.full(n, -1, np.int32), overlap_pos=np.full(n, -1, np.int32), self_score=np.zeros(n),
             vertex_state=np.zeros(nv, np.uint32), nodes=np.zeros(nv, FNO_READ_DTYPE), srs=np.zeros(n, FNO_READ_DTYPE), sr_clique=np.zeros(n, np.uint32),
             clique_off=np.zeros(n + 1, np.uint64), clique_nodes=np.zeros(2 * n_items, np.uint64), subread_off=np.zeros(n + 1, np.uint64),
             subreads=np.zeros(n_items, FNO_SUBREAD_DTYPE))
    out = hc_sr_clique_next_output()
    for k, v in o.items():
        setattr(out, k, v.ctypes.data)  # (an empty numpy array still has an address)
    return a, inp, st, o, out


def _result(o, out, empty, reads=None):
    ns = int(out.n_srs)
    nc, nsub = int(o["clique_off"][ns]), int(o["subread_off"][ns])
    return CliqueNext(o["clique_kind"], o["clique_new_id"], o["overlap_pos"], o["self_score"], o["vertex_state"], o["nodes"], o["srs"][:ns],
                      o["sr_clique"][:ns], o["clique_off"][:ns + 1], o["clique_nodes"][:nc], o["subread_off"][:ns + 1], o["subreads"][:nsub],
                      int(out.n_singles), int(out.n_trivials), int(out.n_paired), int(out.n_self_merged), int(out.new_read_count), out.counts.as_dict(),
                      {k: getattr(out.self_stats, k) for k, _ in out.self_stats._fields_}, float(out.ms_device), float(out.ms_copy), empty, reads)


def clique_next(ctx, clique_off, clique_nodes, merged, vertex_read, vertex_fwd, keep_singletons=0, self_overlap=True, min_score=0.99, min_qual=0.99,
                min_overlap=15, n_threads=16):
    """hc_sr_clique_next on a context (EdgeScorer.sr_clique_next)."""
    keep, inp, st, o, out = _prepare(clique_off, clique_nodes, merged, vertex_read, vertex_fwd, keep_singletons, self_overlap, min_score, min_qual,
                                     min_overlap, n_threads)
    rc = N.lib.hc_sr_clique_next(ctx, C.byref(inp), C.byref(st), C.byref(out))
    if rc not in (0, NEXT_EMPTY):
        N.check(rc, "hc_sr_clique_next")
    return _result(o, out, rc == NEXT_EMPTY)


def host_clique_next(reads, cons_seq, cons_qual, clique_off, clique_nodes, merged, vertex_read, vertex_fwd, settings=None, keep_singletons=0,
                     self_overlap=True, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=1):
    """hc_host_sr_clique_next: the host mirror.  reads: the current ReadSet; cons_seq / cons_qual: the kept consensus bytes; settings: a
    records.Settings, of which --mismatch and --min_read_len are read (the self-overlap test)."""
    from .records import Settings

    keep, inp, st, o, out = _prepare(clique_off, clique_nodes, merged, vertex_read, vertex_fwd, keep_singletons, self_overlap, min_score, min_qual,
                                     min_overlap, n_threads)
    cs = (settings or Settings()).to_c()
    cons_seq, cons_qual = _c(cons_seq, np.uint8), _c(cons_qual, np.uint8)
    if cons_seq.size != cons_qual.size:
        raise ValueError("cons_seq and cons_qual differ in length")
    n = int(inp.n_cliques + inp.n_vertices)
    off, first = np.zeros(2 * n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    nb = C.c_uint64()

    def once(ob, oq, cap):
        return N.lib.hc_host_sr_clique_next(C.byref(cs), _ptr(reads.bases), _ptr(reads.quals), reads.seq_off.ctypes.data, reads.read_first_seq.ctypes.data,
                                            reads.n_reads, _ptr(cons_seq), _ptr(cons_qual), cons_seq.size, C.byref(inp), C.byref(st), C.byref(out), _ptr(ob),
                                            _ptr(oq), cap, C.byref(nb), off.ctypes.data, first.ctypes.data)

    rc = once(None, None, 0)  # count ...
    if rc == NEXT_EMPTY:
        return _result(o, out, True)
    if rc != 0 and out.counts.n_kept == 0:
        N.check(rc, "hc_host_sr_clique_next")
    ob, oq = np.zeros(nb.value, np.uint8), np.zeros(nb.value, np.uint8)
    N.check(once(ob, oq, ob.size), "hc_host_sr_clique_next")  # ... then fetch
    nr, ns = int(out.counts.n_kept), int(out.counts.n_seq)
    return _result(o, out, False, ReadSet(ob, oq, off[:ns + 1], first[:nr + 1], np.arange(nr, dtype=np.uint64)))


@dataclass
class CliqueSelection:
    clique_off: np.ndarray   # uint64, n_selected + 1
    clique_nodes: np.ndarray  # uint32: the accepted cliques, filtered, in file order
    index: np.ndarray        # uint64: the index of each in the input
    n_singletons: int


def host_clique_select(clique_off, clique_nodes, n_vertices, min_clique_size=2, remove_multi_occ=False):
    """hc_host_sr_clique_select: the gate of src/SRBuilder.cpp:1056-1084 over a CSR of cliques in file order."""
    off, nodes = _c(clique_off, np.uint64), _c(clique_nodes, np.uint32)
    if off.size == 0:
        off = np.zeros(1, np.uint64)
    n = off.size - 1
    if nodes.size < int(off[-1]):
        raise ValueError("fewer clique vertices than clique_off names")
    so, sn, si = np.zeros(n + 1, np.uint64), np.zeros(max(int(off[-1]), 1), np.uint32), np.zeros(max(n, 1), np.uint64)
    ns, n1 = C.c_uint64(), C.c_uint64()
    N.check(N.lib.hc_host_sr_clique_select(off.ctypes.data, _ptr(nodes), n, int(n_vertices), int(min_clique_size), int(bool(remove_multi_occ)),
                                           so.ctypes.data, sn.ctypes.data, si.ctypes.data, C.byref(ns), C.byref(n1)), "hc_host_sr_clique_select")
    k = int(ns.value)
    return CliqueSelection(so[:k + 1], sn[:int(so[k])], si[:k], int(n1.value))
