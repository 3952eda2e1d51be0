"""Read evidence for branching edges (include/hcsr.h: hc_br_* and the host mirror hc_host_br_evidence): the first half of
BranchReduction::readBasedBranchReduction — findBranchingEvidence with buildDiffListOut, buildDiffListIn, findDiffPos and checkReadEvidence
(reference src/BranchReduction.cpp:229-743), for every in-branch and then every out-branch (:60-80).  Structures, dtypes and the plumbing
shared by EdgeScorer.br_* (device) and host.br_evidence (the mirror)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .originals import ORIGINAL_DTYPE

_vp = C.c_void_p

BRANCH_DTYPE = np.dtype([("node", "<u4"), ("side", "u1"), ("status", "u1"), ("is_false", "u1"), ("pad", "u1"), ("dist", "<i4"), ("nb_count", "<u4"),
                         ("nb_first", "<u8"), ("diff_first", "<u8"), ("diff_count", "<u4"), ("n_neighbours", "<u4")])
assert BRANCH_DTYPE.itemsize == 40

BR_IN, BR_OUT = 0, 1                                                                          # HC_BR_IN / HC_BR_OUT
BR_OK, BR_PAIRED_NEIGHBOUR, BR_REPEATED_NEIGHBOUR, BR_BAD_GEOMETRY, BR_BAD_ORIGINAL = range(5)  # HC_BR_*
SOME_FAILED = 1                                                                               # HC_BR_SOME_FAILED
MAX_DIFFS = 100                                                                               # HC_BR_MAX_DIFFS


class hc_br_settings(C.Structure):
    _fields_ = [("se_count", C.c_uint64), ("pe_count", C.c_uint64), ("original_readcount", C.c_uint64), ("min_overlap_len", C.c_uint32),
                ("reserved", C.c_uint32), ("edge_threshold", C.c_double)]


class hc_br_counts(C.Structure):
    _fields_ = [("n_branches", C.c_uint64), ("n_branch_nb", C.c_uint64), ("n_diff", C.c_uint64), ("n_ev_edges", C.c_uint64), ("n_ev_ids", C.c_uint64),
                ("n_missing", C.c_uint64), ("n_items", C.c_uint64), ("n_failed", C.c_uint64), ("ms_device", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class hc_br_tables(C.Structure):
    _fields_ = [("branches", _vp), ("cap_branches", C.c_uint64), ("branch_nb", _vp), ("cap_branch_nb", C.c_uint64), ("diff_pos", _vp),
                ("cap_diff", C.c_uint64), ("ev_edge", _vp), ("ev_off", _vp), ("cap_ev_edges", C.c_uint64), ("ev_ids", _vp), ("cap_ev_ids", C.c_uint64),
                ("missing_edges", _vp), ("cap_missing", C.c_uint64)]


class hc_br_host_input(C.Structure):
    _fields_ = [("edges", _vp), ("out_off", _vp), ("in_nodes", _vp), ("in_off", _vp), ("n_vertices", C.c_uint64), ("bases", _vp), ("seq_off", _vp),
                ("read_first_seq", _vp), ("n_reads", C.c_uint64), ("orig_off", _vp), ("entries", _vp), ("original_bases", _vp), ("original_seq_off", _vp),
                ("n_original_reads", C.c_uint64), ("vertex_read", _vp), ("vertex_fwd", _vp)]


for _name, _args in (("hc_br_set_original_reads", [_vp, _vp, _vp, C.c_uint64]),
                     ("hc_br_evidence", [_vp, _vp, _vp, C.c_uint64, C.POINTER(hc_br_settings), C.POINTER(hc_br_counts)]),
                     ("hc_br_evidence_fetch", [_vp, C.POINTER(hc_br_tables)]),
                     ("hc_host_br_evidence", [C.POINTER(hc_br_host_input), C.POINTER(hc_br_settings), C.POINTER(hc_br_counts), C.POINTER(hc_br_tables),
                                              C.c_uint32])):
    getattr(N.lib, _name).restype = C.c_int
    getattr(N.lib, _name).argtypes = _args


@dataclass
class BranchEvidence:
    """The tables of one call, as include/hcsr.h: hc_br_tables describes them."""
    branches: np.ndarray       # BRANCH_DTYPE: in-branches in ascending vertex, then out-branches
    branch_nb: np.ndarray      # uint32: the final_branch neighbours, branch by branch
    diff_pos: np.ndarray       # int32: the diff lists, branch by branch
    ev_edge: np.ndarray        # uint32 (n, 2): evidence_per_edge's keys in ascending (u, v)
    ev_off: np.ndarray         # uint64, n + 1
    ev_ids: np.ndarray         # uint32, ascending inside an edge
    missing_edges: np.ndarray  # host.EDGE_DTYPE, in push order
    counts: dict

    def neighbours(self, b):
        r = self.branches[b]
        return self.branch_nb[int(r["nb_first"]):int(r["nb_first"]) + int(r["nb_count"])]

    def diffs(self, b):
        r = self.branches[b]
        return self.diff_pos[int(r["diff_first"]):int(r["diff_first"]) + int(r["diff_count"])]

    def evidence(self):
        """{(u, v): [ids]}"""
        return {(int(u), int(v)): self.ev_ids[int(self.ev_off[k]):int(self.ev_off[k + 1])].tolist() for k, (u, v) in enumerate(self.ev_edge)}


def settings(se_count, pe_count, original_readcount, min_overlap_len, edge_threshold):
    return hc_br_settings(int(se_count), int(pe_count), int(original_readcount), int(min_overlap_len), 0, float(edge_threshold))


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _tables(cn):
    from .host import EDGE_DTYPE

    a = dict(branches=np.zeros(cn.n_branches, BRANCH_DTYPE), branch_nb=np.zeros(cn.n_branch_nb, np.uint32), diff_pos=np.zeros(cn.n_diff, np.int32),
             ev_edge=np.zeros((cn.n_ev_edges, 2), np.uint32), ev_off=np.zeros(cn.n_ev_edges + 1, np.uint64), ev_ids=np.zeros(cn.n_ev_ids, np.uint32),
             missing_edges=np.zeros(cn.n_missing, EDGE_DTYPE))
    # (every table is wanted: a pointer to at least one element, so that an empty table is not "not wanted"; the stand-ins stay alive in `a`)
    a["_stand_ins"] = {k: np.zeros(1, v.dtype) for k, v in a.items() if v.size == 0}
    p = {k: (a["_stand_ins"][k] if k in a["_stand_ins"] else v).ctypes.data for k, v in a.items() if k != "_stand_ins"}
    t = hc_br_tables(p["branches"], cn.n_branches, p["branch_nb"], cn.n_branch_nb, p["diff_pos"], cn.n_diff, p["ev_edge"], a["ev_off"].ctypes.data,
                     cn.n_ev_edges, p["ev_ids"], cn.n_ev_ids, p["missing_edges"], cn.n_missing)
    return a, t


def set_original_reads(ctx, bases, seq_off):
    bases, seq_off = _c(bases, np.uint8), _c(seq_off, np.uint64)
    if seq_off.size == 0:
        seq_off = np.zeros(1, np.uint64)
    if bases.size < int(seq_off[-1]):
        raise ValueError("fewer bases than seq_off names")
    N.check(N.lib.hc_br_set_original_reads(ctx, _ptr(bases), seq_off.ctypes.data, seq_off.size - 1), "hc_br_set_original_reads")


def evidence(ctx, vertex_read, vertex_fwd, st):
    """hc_br_evidence on a context -> the counts as a dict (with "some_failed")."""
    vr, vf = _c(vertex_read, np.uint32), _c(vertex_fwd, np.uint8)
    if vr.size != vf.size:
        raise ValueError("vertex_read and vertex_fwd differ in length")
    cn = hc_br_counts()
    rc = N.lib.hc_br_evidence(ctx, _ptr(vr), _ptr(vf), vr.size, C.byref(st), C.byref(cn))
    if rc not in (0, SOME_FAILED):
        N.check(rc, "hc_br_evidence")
    return dict(cn.as_dict(), some_failed=rc == SOME_FAILED), cn


def fetch(ctx, cn):
    a, t = _tables(cn)
    N.check(N.lib.hc_br_evidence_fetch(ctx, C.byref(t)), "hc_br_evidence_fetch")
    a.pop("_stand_ins")
    return BranchEvidence(counts=cn.as_dict(), **a)


def host_evidence(graph, reads, orig_off, entries, original_bases, original_seq_off, vertex_read, vertex_fwd, st, n_threads=1, counts=None):
    """hc_host_br_evidence: the mirror.  graph: a dict as EdgeScorer.graph_fetch returns it (edges, out_off, in_nodes, in_off); reads: a ReadSet;
    (orig_off, entries): the dict over its reads; the original reads as set_original_reads takes them.  counts: a hc_br_counts known
    to hold the sizes (an earlier call's), for one call instead of count, then fetch."""
    from .host import EDGE_DTYPE

    keep = dict(edges=_c(graph["edges"], EDGE_DTYPE), out_off=_c(graph["out_off"], np.uint64), in_nodes=_c(graph["in_nodes"], np.uint32),
                in_off=_c(graph["in_off"], np.uint64), bases=_c(reads.bases, np.uint8), seq_off=_c(reads.seq_off, np.uint64),
                read_first_seq=_c(reads.read_first_seq, np.uint32), orig_off=_c(orig_off, np.uint64), entries=_c(entries, ORIGINAL_DTYPE),
                original_bases=_c(original_bases, np.uint8), original_seq_off=_c(original_seq_off, np.uint64), vertex_read=_c(vertex_read, np.uint32),
                vertex_fwd=_c(vertex_fwd, np.uint8))
    V = keep["out_off"].size - 1
    if keep["in_off"].size != V + 1 or keep["vertex_read"].size != V or keep["vertex_fwd"].size != V:
        raise ValueError("the per-vertex arrays differ in length")
    if keep["orig_off"].size != reads.n_reads + 1 or keep["entries"].size < int(keep["orig_off"][-1]):
        raise ValueError("the dict is not one over the reads of the store")
    inp = hc_br_host_input()
    for k, v in keep.items():
        setattr(inp, k, _ptr(v))
    for k in ("out_off", "in_off", "seq_off", "read_first_seq", "orig_off", "original_seq_off"):
        setattr(inp, k, keep[k].ctypes.data)
    inp.n_vertices, inp.n_reads, inp.n_original_reads = V, reads.n_reads, keep["original_seq_off"].size - 1
    cn = hc_br_counts()
    if counts is None:
        rc = N.lib.hc_host_br_evidence(C.byref(inp), C.byref(st), C.byref(cn), None, int(n_threads))  # count ...
        if rc not in (0, SOME_FAILED):
            N.check(rc, "hc_host_br_evidence")
    a, t = _tables(cn if counts is None else counts)
    rc = N.lib.hc_host_br_evidence(C.byref(inp), C.byref(st), C.byref(cn), C.byref(t), int(n_threads))  # ... then fetch
    if rc not in (0, SOME_FAILED):
        N.check(rc, "hc_host_br_evidence")
    a.pop("_stand_ins")
    return BranchEvidence(counts=dict(cn.as_dict(), some_failed=rc == SOME_FAILED), **a)
