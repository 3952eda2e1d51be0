"""Read evidence for branching edges (include/hcsr.h: hc_br_* and the host mirror hc_host_br_evidence): the first half of
BranchReduction::readBasedBranchReduction — findBranchingEvidence with buildDiffListOut, buildDiffListIn, findDiffPos and checkReadEvidence
(reference src/BranchReduction.cpp:229-743), for every in-branch and then every out-branch (:60-80).  Structures, dtypes and the plumbing
shared by EdgeScorer.br_* (device) and host.br_evidence (the mirror).  Behind them the second half (:82-227, :745-1272): reduce() /
reduce_fetch() on a context, host_reduce() (the mirror hc_host_br_reduce) and parse_thresholds()."""
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


# ---- the reduction: hc_br_reduce / hc_br_reduce_fetch / hc_host_br_reduce / hc_host_br_parse_thresholds ---------------------------------

COMPONENT_DTYPE = np.dtype([("dist", "<i4"), ("min_evidence", "<i4"), ("outcome", "<u4"), ("host_finished", "<u4"), ("edge_first", "<u8"),
                            ("edge_count", "<u4"), ("pad", "<u4")])
assert COMPONENT_DTYPE.itemsize == 32
THRESHOLD_DTYPE = np.dtype([("dist", "<i4"), ("min_evidence", "<i4")])

RED_KEPT, RED_NOT_KEPT, RED_NO_THRESHOLD, RED_CAREFUL = range(4)        # HC_BR_RED_*
RED_HOST_NO_ROW, RED_HOST_SHARED_EDGE, RED_HOST_DIPLOID = 1, 2, 4       # HC_BR_RED_HOST_*

for _name, _args in (("hc_br_reduce", [_vp, C.POINTER(N.hc_br_reduce_settings), C.POINTER(N.hc_br_reduce_counts)]),
                     ("hc_br_reduce_fetch", [_vp, C.POINTER(N.hc_br_reduce_tables)]),
                     ("hc_host_br_reduce", [C.POINTER(hc_br_host_input), C.POINTER(hc_br_tables), C.POINTER(N.hc_br_reduce_settings),
                                            C.POINTER(N.hc_br_reduce_counts), C.POINTER(N.hc_br_reduce_tables), C.POINTER(N.hc_br_host_graph_out)]),
                     ("hc_host_br_parse_thresholds", [C.c_char_p, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
                     ("hc_host_br_map_order", [C.c_uint64, _vp])):
    getattr(N.lib, _name).restype = C.c_int
    getattr(N.lib, _name).argtypes = _args


@dataclass
class BranchReduction:
    """The tables of one reduction, as include/hcsr.h: hc_br_reduce_tables describes them."""
    components: np.ndarray   # COMPONENT_DTYPE, in branching_components order
    comp_edge: np.ndarray    # uint32 (n, 2), component by component
    comp_unique: np.ndarray  # uint32 per comp_edge row
    removed: np.ndarray      # uint32 (n, 2): edges_to_remove, sorted and unique
    counts: dict

    def component_edges(self, i):
        c = self.components[i]
        return self.comp_edge[int(c["edge_first"]):int(c["edge_first"]) + int(c["edge_count"])]


def reduce_settings(thresholds, careful=False, diploid=True):
    """thresholds: {dist: min_evidence}, or an array of THRESHOLD_DTYPE (parse_thresholds' result).  Returns (settings, what it points into)."""
    if isinstance(thresholds, dict):
        t = np.array(sorted(thresholds.items()), np.int32).reshape(-1, 2).copy().view(THRESHOLD_DTYPE).reshape(-1)
    else:
        t = _c(thresholds, THRESHOLD_DTYPE)
    return N.hc_br_reduce_settings(int(bool(careful)), int(bool(diploid)), 0, 0, _ptr(t), t.size), t


def parse_thresholds(text):
    """hc_host_br_parse_thresholds: the bytes of an evidence_threshold_table.tsv -> THRESHOLD_DTYPE in ascending dist.  A line std::stoi would
    throw on raises HcError with .bad_line (1-based)."""
    if isinstance(text, str):
        text = text.encode()
    n, bad = C.c_uint64(0), C.c_uint64(0)
    out = np.zeros(text.count(b"\n") + 1, THRESHOLD_DTYPE)
    rc = N.lib.hc_host_br_parse_thresholds(text, len(text), out.ctypes.data, out.size, C.byref(n), C.byref(bad))
    if rc:
        try:
            N.check(rc, "hc_host_br_parse_thresholds")
        except N.HcError as e:
            e.bad_line = int(bad.value)
            raise
    return out[:n.value].copy()


def map_order(n):
    """hc_host_br_map_order: the iteration order of the library's std::unordered_map< node_id_t, bool > after inserting 0 .. n - 1."""
    out = np.zeros(max(n, 1), np.uint64)
    N.check(N.lib.hc_host_br_map_order(n, out.ctypes.data), "hc_host_br_map_order")
    return out[:n].tolist()


def _reduce_tables(n_components, n_comp_edges, n_removed):
    a = dict(components=np.zeros(max(n_components, 1), COMPONENT_DTYPE), comp_edge=np.zeros((max(n_comp_edges, 1), 2), np.uint32),
             comp_unique=np.zeros(max(n_comp_edges, 1), np.uint32), removed=np.zeros((max(n_removed, 1), 2), np.uint32))
    t = N.hc_br_reduce_tables(a["components"].ctypes.data, a["components"].size, a["comp_edge"].ctypes.data, a["comp_unique"].ctypes.data,
                              a["comp_unique"].size, a["removed"].ctypes.data, a["removed"].shape[0])
    return a, t


def _reduction(a, cn):
    return BranchReduction(a["components"][:cn.n_components].copy(), a["comp_edge"][:cn.n_component_edges].copy(),
                           a["comp_unique"][:cn.n_component_edges].copy(), a["removed"][:cn.n_removed].copy(), cn.as_dict())


def reduce(ctx, settings):
    """hc_br_reduce on a context -> (counts as a dict, the counts structure)."""
    st, keep = settings
    cn = N.hc_br_reduce_counts()
    N.check(N.lib.hc_br_reduce(ctx, C.byref(st), C.byref(cn)), "hc_br_reduce")
    del keep
    return cn.as_dict(), cn


def reduce_fetch(ctx, cn):
    a, t = _reduce_tables(cn.n_components, cn.n_component_edges, cn.n_removed)
    N.check(N.lib.hc_br_reduce_fetch(ctx, C.byref(t)), "hc_br_reduce_fetch")
    return _reduction(a, cn)


def host_reduce(graph, reads, ev, settings):
    """hc_host_br_reduce: the mirror.  graph: a dict as EdgeScorer.graph_fetch returns it; reads: a ReadSet; ev: a BranchEvidence; settings:
    reduce_settings(...).  Returns (BranchReduction, the reduced graph as such a dict, the records appended to branching_edges)."""
    from .host import EDGE_DTYPE

    st, keep_t = settings
    keep = dict(edges=_c(graph["edges"], EDGE_DTYPE), out_off=_c(graph["out_off"], np.uint64), in_nodes=_c(graph["in_nodes"], np.uint32),
                in_off=_c(graph["in_off"], np.uint64), bases=_c(reads.bases, np.uint8), seq_off=_c(reads.seq_off, np.uint64),
                read_first_seq=_c(reads.read_first_seq, np.uint32))
    V, E = keep["out_off"].size - 1, keep["edges"].size
    inp = hc_br_host_input()
    for k, v in keep.items():
        setattr(inp, k, _ptr(v))
    for k in ("out_off", "in_off", "seq_off", "read_first_seq"):
        setattr(inp, k, keep[k].ctypes.data)
    inp.n_vertices, inp.n_reads = V, reads.n_reads
    tk = dict(branches=_c(ev.branches, BRANCH_DTYPE), branch_nb=_c(ev.branch_nb, np.uint32), ev_edge=_c(ev.ev_edge, np.uint32), ev_off=_c(ev.ev_off, np.uint64),
              ev_ids=_c(ev.ev_ids, np.uint32), missing_edges=_c(ev.missing_edges, EDGE_DTYPE))
    n_rows = tk["ev_off"].size - 1
    t = hc_br_tables(_ptr(tk["branches"]), tk["branches"].size, _ptr(tk["branch_nb"]), tk["branch_nb"].size, None, 0, _ptr(tk["ev_edge"]),
                     tk["ev_off"].ctypes.data, n_rows, _ptr(tk["ev_ids"]), tk["ev_ids"].size, _ptr(tk["missing_edges"]), tk["missing_edges"].size)
    a, rt = _reduce_tables(tk["branches"].size, tk["branch_nb"].size, tk["branch_nb"].size)  # the upper bounds: one call
    g = dict(edges=np.zeros(max(E, 1), EDGE_DTYPE), out_off=np.zeros(V + 1, np.uint64), in_nodes=np.zeros(max(E, 1), np.uint32), in_off=np.zeros(V + 1, np.uint64))
    br = np.zeros(max(E + tk["missing_edges"].size, 1), EDGE_DTYPE)
    go = N.hc_br_host_graph_out(g["edges"].ctypes.data, g["edges"].size, g["out_off"].ctypes.data, g["in_nodes"].ctypes.data, g["in_off"].ctypes.data,
                                br.ctypes.data, br.size, 0, 0)
    cn = N.hc_br_reduce_counts()
    N.check(N.lib.hc_host_br_reduce(C.byref(inp), C.byref(t), C.byref(st), C.byref(cn), C.byref(rt), C.byref(go)), "hc_host_br_reduce")
    del keep_t
    g["edges"], g["in_nodes"] = g["edges"][:go.n_edges].copy(), g["in_nodes"][:go.n_edges].copy()
    return _reduction(a, cn), g, br[:go.n_branching].copy()
