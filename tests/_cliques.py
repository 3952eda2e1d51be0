"""Shared by the clique tests: the cases of tests/golden/cliques.json (quick-cliques' own output, made by
tests/golden/make_golden_cliques.py) as graphs, a restatement in Python of the order rule of hc_graph_cliques (include/hcedge.h), an
exhaustive enumerator for small graphs, and graph builders."""
import base64
import functools
import json
import os
import struct
import zlib

import numpy as np

from tests import _trans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cliques.json")


def _unpack(case):
    """A graph the golden script built, unpacked into the fields of the others (the file's note describes the packing)."""
    V = case["n_vertices"]
    raw = zlib.decompress(base64.b64decode(case.pop("pairs_z")))
    vals = struct.unpack(f"<{len(raw) // 2}H", raw)
    edges, k = [], V
    for a in range(V):
        b = a
        for _ in range(vals[a]):
            b += vals[k]
            k += 1
            edges.append([a, b] if (a + b) & 1 else [b, a])
    case["edges"], case["inclusions"] = edges, [0] * V
    case["qc_stdout"] = zlib.decompress(base64.b64decode(case.pop("qc_stdout_z"))).decode().split("\n")
    return case


@functools.lru_cache(maxsize=None)
def load_cases():
    with open(GOLDEN) as f:
        return [_unpack(c) if "pairs_z" in c else c for c in json.load(f)["cases"]]


def qc_cliques(lines):
    """The cliques among qc's stdout lines (a line of integers each), as a list of sorted tuples; and the other lines."""
    out, text = [], []
    for ln in lines:
        tok = ln.split()
        if tok and all(t.isdigit() for t in tok):
            out.append(tuple(sorted(int(t) for t in tok)))
        else:
            text.append(ln)
    return out, text


def graph(V, pairs, incl=None, seed=1):
    """(edges, out_off, in_nodes, in_off, inclusions) of out-records v1 -> v2 in insertion order."""
    v1 = np.array([p[0] for p in pairs], np.int64)
    v2 = np.array([p[1] for p in pairs], np.int64)
    r = _trans.make_records(v1, v2, seed)
    return (*_trans.csr_from_inserts(r, V), np.zeros(V, np.uint8) if incl is None else np.asarray(incl, np.uint8))


def case_graph(case):
    return graph(case["n_vertices"], case["edges"], case["inclusions"])


def pair_set(V, pairs, incl=None):
    """The undirected pairs writeGraphToFile's loops describe (src/OverlapGraph.cpp:322-385), each once."""
    incl = [0] * V if incl is None else incl
    return {(min(a, b), max(a, b)) for a, b in pairs if not incl[a] and not incl[b]}


def restate(V, pairs):
    """The rule of include/hcedge.h, restated: a list of cliques (ascending vertex lists) in the call's order."""
    nb = [set() for _ in range(V)]
    for a, b in pairs:
        nb[a].add(b)
        nb[b].add(a)
    order = sorted(range(V), key=lambda v: (len(nb[v]), v))  # 1. rank = the position in ascending (degree, id)
    rank = {v: r for r, v in enumerate(order)}
    out = []
    for v in order:  # 3. roots in ascending rank
        loc = sorted(nb[v])  # 4. local indices: the neighbours in ascending id
        P = {a for a, u in enumerate(loc) if rank[u] > rank[v]}
        X = set(range(len(loc))) - P
        if not P:
            if not X:
                out.append([v])
            continue
        adj = [{b for b, w in enumerate(loc) if w in nb[u]} for u in loc]

        def bk(R, P, X):
            if not P:
                if not X:
                    out.append(sorted([v] + [loc[a] for a in R]))  # 5.
                return
            pivot = max(sorted(P | X), key=lambda u: (len(adj[u] & P), -u))  # most neighbours in P, ties to the smallest index
            for c in sorted(P - adj[pivot]):
                bk(R | {c}, P & adj[c], X & adj[c])
                P = P - {c}
                X = X | {c}

        bk(set(), P, X)
    return out


def csr(cliques):
    off = np.zeros(len(cliques) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in cliques])
    return off, np.array([x for c in cliques for x in c], np.uint32)


def exhaustive(V, pairs):
    """Every maximal clique of a graph of at most 14 vertices, by testing every subset."""
    assert 0 < V <= 14
    adj = np.zeros(V, np.int64)
    for a, b in pairs:
        adj[a] |= 1 << b
        adj[b] |= 1 << a
    masks = np.arange(1, 1 << V, dtype=np.int64)
    is_clique = np.ones(masks.size, bool)
    extendable = np.zeros(masks.size, bool)
    for v in range(V):
        member = (masks >> v & 1) == 1
        all_adjacent = (masks & ~adj[v] & ~(1 << v)) == 0
        is_clique &= ~member | all_adjacent
        extendable |= ~member & all_adjacent
    return {tuple(v for v in range(V) if m >> v & 1) for m in masks[is_clique & ~extendable]}


def complete(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def complete_minus_matching(n, first=0):
    """K_n without the pairs {0,1}, {2,3}, ...: 2^(n/2) maximal cliques."""
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n) if not (a ^ 1) == b]


def interval_pairs(V, reach, seed, spread=8):
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, V * spread, V))
    hi = np.searchsorted(pos, pos + reach, side="left")
    return [(i, j) for i in range(V) for j in range(i + 1, int(hi[i]))]


def overlap_graph(n=60, seed=5):
    """A store of n single-end forward reads cut from one template at rising offsets, and its overlap graph: i -> j for every pair whose
    starts are less than 60 bases apart, pos1 = the distance, records in shuffled order.  Every maximal clique has three to five reads
    and a consistent layout.  -> (reads, V, rows in tests/_edge_merge.py: csr's form, vertex_read, vertex_fwd)"""
    from haploconduct_amd.readstore import ReadSet

    rng = np.random.default_rng(seed)
    tmpl = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 40 * n + 200)]
    a = np.cumsum(rng.integers(5, 26, n))
    length = rng.integers(90, 131, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(length)
    reads = ReadSet(np.concatenate([tmpl[a[k]:a[k] + length[k]] for k in range(n)]), rng.integers(50, 74, int(length.sum())).astype(np.uint8), off,
                    np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint64))
    rows = [[i, j, i, j, int(a[j] - a[i]), 0, 1, 1, ord("1")] for i in range(n) for j in range(i + 1, n) if a[j] - a[i] < 60]
    return reads, n, [rows[k] for k in rng.permutation(len(rows))], np.arange(n, dtype=np.uint32), np.ones(n, np.uint8)
