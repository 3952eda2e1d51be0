"""Shared by the cycle-removal tests: the cases of tests/golden/cycles.json (the reference's own sortEdges, findCycles and
cycleRemovalHeuristic, made by tests/golden/make_golden_cycles.py) as graphs, graph builders, and the host mirror's chain."""
import functools
import json
import os

import numpy as np

from haploconduct_amd import cycles as CY
from haploconduct_amd.host import EDGE_DTYPE
from tests import _trans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cycles.json")
ALL_FIELDS = ("v1", "v2", "read1", "read2", "pos1", "pos2", "pos3", "pos4", "ori1", "ori2", "ord", "perc", "score", "mismatch_rate", "len0", "len1", "len2")
COUNTS = ("edges_before", "edges_after", "backedge_count", "tries", "best_try", "try_size", "n_flagged_components", "n_host_vertices", "n_host_edges",
          "status", "bad_v", "bad_pos")


@functools.lru_cache(maxsize=None)
def load():
    with open(GOLDEN) as f:
        g = json.load(f)
    for c in g["cases"]:  # the input records are stored as rows
        c["edges"] = [dict(zip(g["edge_fields"], row)) for row in c["edges"]]
    return g


def records(v1, v2, pos1=5, len1=30, score=1.0, mismatch_rate=0.25):
    """Full records with the encoding of make_golden_cycles.py: read = vertex, len0 = len1, perc = the record's index.  Arrays or scalars."""
    v1 = np.asarray(v1, np.uint64)
    r = np.zeros(v1.size, EDGE_DTYPE)
    r["v1"], r["v2"], r["pos1"], r["len1"], r["score"], r["mismatch_rate"] = v1, v2, pos1, len1, score, mismatch_rate
    r["read1"], r["read2"], r["len0"], r["perc"] = r["v1"], r["v2"], r["len1"], np.arange(v1.size)
    r["ori1"], r["ori2"], r["ord"] = 1, 1, ord("-")
    return r


def case_records(edges):
    cols = {f: [e[f] for e in edges] for f in ("v1", "v2", "pos1", "len1", "score", "mismatch_rate")}
    return records(**cols) if edges else np.zeros(0, EDGE_DTYPE)


def inserted(V, recs):
    """(records, out_off, in_nodes, in_off) of the graph addEdge calls in the given order leave."""
    return _trans.csr_from_inserts(recs, V)


def out_offsets(edges, V):
    off = np.zeros(V + 1, np.uint64)
    np.add.at(off, edges["v1"].astype(np.int64) + 1, 1)
    return np.cumsum(off).astype(np.uint64)


def host_sorted(g, lens):
    """hc_host_graph_sort_edges on a graph: (edges, out_off, in_nodes, in_off)."""
    m = _trans.Mirror(*g)
    m.g.sort_edges(lens)
    edges, in_off, in_nodes = m.result()
    return edges, out_offsets(edges, m.V), in_nodes.astype(np.uint32), in_off


def _field(r, f):  # the doubles by their bits: a NaN equals itself, -0.0 is not +0.0
    return np.ascontiguousarray(r[f]).view(np.uint64) if f in ("score", "mismatch_rate") else r[f]


def same_records(a, b):
    return a.shape == b.shape and all(np.array_equal(_field(a, f), _field(b, f)) for f in ALL_FIELDS)


def same_graph(a, b):
    """(edges, out_off, in_nodes, in_off) equal array for array, every field of the records."""
    return same_records(a[0], b[0]) and all(np.array_equal(np.asarray(x, np.uint64), np.asarray(y, np.uint64)) for x, y in zip(a[1:], b[1:]))


def mirror(g, remove_edges=True, n_threads=1):
    """hc_host_graph_remove_cycles on a graph in sortEdges' order: a cycles.CycleRemoval."""
    return CY.host_remove_cycles(*g, remove_edges=remove_edges, n_threads=n_threads)


def graph_of(r):
    return r.edges, r.out_off, r.in_nodes, r.in_off


def chain(V, closed):
    """i -> i + 1; closed: the record V - 1 -> 0 as well.  Lengths differ, so no list order is left to a tie."""
    n = V if closed else V - 1
    i = np.arange(n)
    return records(i, (i + 1) % V, pos1=i % 7, len1=20 + i % 11, score=(1 + i % 5) / 8.0, mismatch_rate=(i % 3) / 16.0), np.full(V, 100, np.uint32)


def random_records(rng, V, n_edges, lo=0, acyclic=False):
    """Seeded records on [lo, lo + V): keys from few values, so ties are common; acyclic: every record ascends."""
    a, b = rng.integers(0, V, n_edges), rng.integers(0, V, n_edges)
    keep = a != b
    a, b = a[keep], b[keep]
    if acyclic:
        a, b = np.minimum(a, b), np.maximum(a, b)
    n = a.size
    return records(lo + a, lo + b, pos1=rng.integers(-4, 6, n), len1=rng.integers(20, 40, n), score=rng.integers(1, 9, n) / 8.0,
                   mismatch_rate=rng.integers(0, 9, n) / 64.0)


def concat(parts):
    r = np.concatenate(parts)
    r["perc"] = np.arange(r.size)
    return r
