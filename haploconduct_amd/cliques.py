"""Maximal cliques of the overlap graph (include/hcedge.h: hc_graph_cliques / hc_graph_cliques_fetch, and the host mirror
hc_host_graph_cliques): what the reference gets from quick-cliques on graph.txt (src/ViralQuasispecies.cpp:397-410), as a CSR of vertex
ids in the call's own order — the arrays hc_host_sr_clique_select and hc_sr_clique_merge take.  Structures, result type and the
plumbing shared by EdgeScorer.graph_cliques (device) and host_graph_cliques (the mirror)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N

_vp = C.c_void_p

CLIQUES_STATUS = ("OK", "SELF_LOOP", "INCLUSION_HAS_EDGES", "OVER_BUDGET")  # HC_CLIQUES_*
DEFAULT_ROOT_CAP = 1024  # HC_CLIQUES_DEFAULT_ROOT_CAP
MAX_ROOT_CAP = 2048      # HC_CLIQUES_MAX_ROOT_CAP: a larger root_cap is taken as this


class hc_cliques_settings(C.Structure):
    _fields_ = [("root_cap", C.c_uint32), ("n_threads", C.c_uint32), ("max_entries", C.c_uint64)]


class hc_cliques_counts(C.Structure):
    _fields_ = [("status", C.c_uint32), ("pad", C.c_uint32)] + \
               [(k, C.c_uint64) for k in ("bad_v", "bad_pos", "n_pairs", "n_cliques", "n_entries", "n_singletons", "max_clique", "n_host_roots")] + \
               [("ms_device", C.c_double), ("ms_host", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


N.lib.hc_graph_cliques.restype = C.c_int
N.lib.hc_graph_cliques.argtypes = [_vp, C.POINTER(hc_cliques_settings), C.POINTER(hc_cliques_counts)]
N.lib.hc_graph_cliques_fetch.restype = C.c_int
N.lib.hc_graph_cliques_fetch.argtypes = [_vp, _vp, _vp]
N.lib.hc_host_graph_cliques.restype = C.c_int
N.lib.hc_host_graph_cliques.argtypes = [_vp, _vp, C.c_uint64, _vp, C.POINTER(hc_cliques_settings), _vp, _vp, C.c_uint64, C.c_uint64,
                                        C.POINTER(hc_cliques_counts)]


@dataclass
class Cliques:
    clique_off: np.ndarray    # uint64, n_cliques + 1
    clique_nodes: np.ndarray  # uint32, ascending inside a clique
    counts: dict              # hc_cliques_counts; counts["status"] != 0: nothing was kept and the arrays are empty

    @property
    def status(self):
        return CLIQUES_STATUS[self.counts["status"]]

    def row(self, k):
        return self.clique_nodes[int(self.clique_off[k]):int(self.clique_off[k + 1])]

    def as_set(self):
        return {tuple(int(x) for x in self.row(k)) for k in range(self.clique_off.size - 1)}


def _none(counts):
    return Cliques(np.zeros(1, np.uint64), np.zeros(0, np.uint32), counts.as_dict())


def graph_cliques(ctx, root_cap=0, max_entries=0, n_threads=16, fetch=True):
    """hc_graph_cliques on a context, then hc_graph_cliques_fetch (fetch=False: the counts alone; the CSR stays on the device)."""
    st, c = hc_cliques_settings(int(root_cap), int(n_threads), int(max_entries)), hc_cliques_counts()
    N.check(N.lib.hc_graph_cliques(ctx, C.byref(st), C.byref(c)), "hc_graph_cliques")
    if c.status != 0 or not fetch:
        return _none(c)
    off, nodes = np.zeros(int(c.n_cliques) + 1, np.uint64), np.zeros(int(c.n_entries), np.uint32)
    N.check(N.lib.hc_graph_cliques_fetch(ctx, off.ctypes.data, nodes.ctypes.data if nodes.size else None), "hc_graph_cliques_fetch")
    return Cliques(off, nodes, c.as_dict())


def host_graph_cliques(edges, out_off, inclusions=None, max_entries=0, n_threads=1):
    """hc_host_graph_cliques: the host mirror on hc_graph_fetch's arrays (count, then fetch)."""
    from .host import EDGE_DTYPE

    e, oo = np.ascontiguousarray(edges, dtype=EDGE_DTYPE), np.ascontiguousarray(out_off, np.uint64)
    inc = None if inclusions is None else np.ascontiguousarray(inclusions, np.uint8)
    V = oo.size - 1
    st, c = hc_cliques_settings(0, int(n_threads), int(max_entries)), hc_cliques_counts()

    def once(off, nodes):
        return N.lib.hc_host_graph_cliques(e.ctypes.data if e.size else None, oo.ctypes.data, V, inc.ctypes.data if inc is not None and inc.size else None,
                                           C.byref(st), None if off is None else off.ctypes.data, None if nodes is None else nodes.ctypes.data,
                                           0 if off is None else off.size - 1, 0 if nodes is None else nodes.size, C.byref(c))

    N.check(once(None, None), "hc_host_graph_cliques")  # count ...
    if c.status != 0:
        return _none(c)
    off, nodes = np.zeros(int(c.n_cliques) + 1, np.uint64), np.zeros(max(int(c.n_entries), 1), np.uint32)
    N.check(once(off, nodes), "hc_host_graph_cliques")  # ... then fetch
    return Cliques(off, nodes[:int(c.n_entries)], c.as_dict())
