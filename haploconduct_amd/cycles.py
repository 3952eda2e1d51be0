"""The second sortEdges of an iteration and cycleRemovalHeuristic (include/hcedge.h: hc_graph_sort_edges, hc_graph_remove_cycles,
hc_graph_fetch_cycle_pairs; include/hcedge_host.h: hc_host_graph_remove_cycles, hc_host_graph_find_cycles): the steps of
src/ViralQuasispecies.cpp:359-367 on the device graph and their host mirror.  Structures, result type and the plumbing shared by
EdgeScorer.graph_sort_edges / graph_remove_cycles (device) and host_remove_cycles / host_find_cycles (the mirror)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N

_vp = C.c_void_p

CYCLES_STATUS = ("OK", "NAN_KEY", "NOT_SORTED")  # HC_CYCLES_*
TRIES = 20  # HC_CYCLES_TRIES


class hc_sort_counts(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_tied_lists", C.c_uint64)]


class hc_cycles_settings(C.Structure):
    _fields_ = [("remove_edges", C.c_uint32), ("pad", C.c_uint32)]


class hc_cycles_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("edges_before", "edges_after", "backedge_count", "tries", "best_try")] + \
               [("try_size", C.c_uint64 * TRIES)] + \
               [(k, C.c_uint64) for k in ("n_flagged_components", "n_host_vertices", "n_host_edges")] + \
               [(k, C.c_uint32) for k in ("status", "bad_v", "bad_pos", "pad")] + \
               [(k, C.c_double) for k in ("ms_first_device", "ms_first_walk", "ms_sub_device", "ms_sub_walk", "ms_edit")]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("pad", "try_size")}
        d["try_size"] = [int(x) for x in self.try_size]
        return d


N.lib.hc_graph_sort_edges.restype = C.c_int
N.lib.hc_graph_sort_edges.argtypes = [_vp, _vp, C.c_uint64, C.POINTER(hc_sort_counts)]
N.lib.hc_graph_remove_cycles.restype = C.c_int
N.lib.hc_graph_remove_cycles.argtypes = [_vp, C.POINTER(hc_cycles_settings), C.POINTER(hc_cycles_counts)]
N.lib.hc_graph_fetch_cycle_pairs.restype = C.c_int
N.lib.hc_graph_fetch_cycle_pairs.argtypes = [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]
N.lib.hc_host_graph_remove_cycles.restype = C.c_int
N.lib.hc_host_graph_remove_cycles.argtypes = [_vp, _vp, _vp, _vp, C.c_uint64, C.POINTER(hc_cycles_settings), C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                              C.c_uint64, C.POINTER(hc_cycles_counts)]
N.lib.hc_host_graph_find_cycles.restype = C.c_int
N.lib.hc_host_graph_find_cycles.argtypes = [_vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]
N.lib.hc_host_cycles_perm_table.restype = C.c_int
N.lib.hc_host_cycles_perm_table.argtypes = [C.c_uint32, _vp]


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


@dataclass
class CycleRemoval:
    pairs: np.ndarray   # uint32 (n, 2): the applied set in ascending (u, v) — the lines of cycles.txt
    counts: dict        # hc_cycles_counts
    edges: np.ndarray = None      # the mirror only: the graph afterwards (EDGE_DTYPE, out_off, in_nodes, in_off) ...
    out_off: np.ndarray = None
    in_nodes: np.ndarray = None
    in_off: np.ndarray = None
    removed: np.ndarray = None    # ... and the records that left, in (u, v) order

    @property
    def status(self):
        return CYCLES_STATUS[self.counts["status"]]

    def cycles_txt(self):
        """The bytes of cycles.txt (reportCycle, src/OverlapGraph.cpp:560), or None where the reference leaves no file."""
        if not self.pairs.shape[0]:
            return None
        return "".join(f"{int(u)}\t{int(v)}\n" for u, v in self.pairs).encode()


def graph_sort_edges(ctx, len_by_read):
    """hc_graph_sort_edges on a context; returns the counts."""
    L = np.ascontiguousarray(len_by_read, np.uint32)
    c = hc_sort_counts()
    N.check(N.lib.hc_graph_sort_edges(ctx, _p(L), L.size, C.byref(c)), "hc_graph_sort_edges")
    return {"n_edges": int(c.n_edges), "n_tied_lists": int(c.n_tied_lists)}


def graph_remove_cycles(ctx, remove_edges=True):
    """hc_graph_remove_cycles on a context, then hc_graph_fetch_cycle_pairs.  A refused graph (HC_ERR_STATE) raises."""
    st, c = hc_cycles_settings(1 if remove_edges else 0, 0), hc_cycles_counts()
    N.check(N.lib.hc_graph_remove_cycles(ctx, C.byref(st), C.byref(c)), "hc_graph_remove_cycles")
    if c.status != 0:
        return CycleRemoval(np.zeros((0, 2), np.uint32), c.as_dict())
    n = C.c_uint64()
    pairs = np.zeros((int(c.backedge_count), 2), np.uint32)
    N.check(N.lib.hc_graph_fetch_cycle_pairs(ctx, _p(pairs), pairs.shape[0], C.byref(n)), "hc_graph_fetch_cycle_pairs")
    return CycleRemoval(pairs, c.as_dict())


def _arrays(edges, out_off, in_nodes, in_off):
    from .host import EDGE_DTYPE

    return (np.ascontiguousarray(edges, dtype=EDGE_DTYPE), np.ascontiguousarray(out_off, np.uint64),
            None if in_nodes is None else np.ascontiguousarray(in_nodes, np.uint32), np.ascontiguousarray(in_off, np.uint64))


def host_remove_cycles(edges, out_off, in_nodes, in_off, remove_edges=True, n_threads=1, cap_pairs=None):
    """hc_host_graph_remove_cycles: the host mirror on hc_graph_fetch's arrays (count, then fetch; with cap_pairs one call with room for
    that many pairs, which raises when there are more)."""
    from .host import EDGE_DTYPE

    e, oo, inn, io = _arrays(edges, out_off, in_nodes, in_off)
    V, E = oo.size - 1, e.shape[0]
    st, c = hc_cycles_settings(1 if remove_edges else 0, 0), hc_cycles_counts()
    head = (_p(e), oo.ctypes.data, _p(inn), io.ctypes.data, V, C.byref(st), int(n_threads))
    if cap_pairs is None:
        N.check(N.lib.hc_host_graph_remove_cycles(*head, None, None, None, None, None, None, 0, C.byref(c)), "hc_host_graph_remove_cycles")  # count ...
    n = int(c.backedge_count) if cap_pairs is None else int(cap_pairs)
    e2, oo2, inn2, io2 = np.zeros(E, EDGE_DTYPE), np.zeros(V + 1, np.uint64), np.zeros(E, np.uint32), np.zeros(V + 1, np.uint64)
    removed, pairs = np.zeros(n, EDGE_DTYPE), np.zeros((n, 2), np.uint32)
    N.check(N.lib.hc_host_graph_remove_cycles(*head, _p(e2), oo2.ctypes.data, _p(inn2), io2.ctypes.data, _p(removed), _p(pairs), n, C.byref(c)),
            "hc_host_graph_remove_cycles")  # ... then fetch
    k, n = int(c.edges_after), int(c.backedge_count)
    pairs = pairs[:n if c.status == 0 else 0]
    removed = removed[:n if remove_edges and c.status == 0 else 0]
    return CycleRemoval(pairs, c.as_dict(), e2[:k], oo2, inn2[:k], io2, removed)


def host_find_cycles(edges, out_off, in_off, t):
    """hc_host_graph_find_cycles: findCycles(t) alone as a uint32 (n, 2) array in ascending (u, v)."""
    e, oo, _, io = _arrays(edges, out_off, None, in_off)
    n = C.c_uint64()
    N.check(N.lib.hc_host_graph_find_cycles(_p(e), oo.ctypes.data, io.ctypes.data, oo.size - 1, int(t), None, 0, C.byref(n)), "hc_host_graph_find_cycles")
    pairs = np.zeros((n.value, 2), np.uint32)
    N.check(N.lib.hc_host_graph_find_cycles(_p(e), oo.ctypes.data, io.ctypes.data, oo.size - 1, int(t), _p(pairs), pairs.shape[0], C.byref(n)),
            "hc_host_graph_find_cycles")
    return pairs


def perm_table(length):
    """hc_host_cycles_perm_table: the 16 permutations (tries 5 .. 20) of a list of `length` records, one row each."""
    t = np.zeros((16, int(length)), np.uint32)
    N.check(N.lib.hc_host_cycles_perm_table(int(length), _p(t)), "hc_host_cycles_perm_table")
    return t
