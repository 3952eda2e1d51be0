"""Shared by the vertex-labelling tests: the cases of tests/golden/labelling.json (the reference's own vertexLabellingHeuristic, made by
tests/golden/make_golden_labelling.py) as graphs, graph builders, and a restatement in Python of the cited lines
(src/GraphAlgos.cpp:150-349, src/Edge.h:90-121, src/OverlapGraph.cpp:94-101, 150-194, 263-282, 578-605, glibc's TYPE_3 rand and
libstdc++'s random_shuffle) over plain lists."""
import base64
import functools
import json
import os

import numpy as np

from haploconduct_amd.host import EDGE_DTYPE
from tests import _trans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labelling.json")
FIELDS = ("v1", "v2", "read1", "read2", "pos1", "pos2", "pos3", "pos4", "ori1", "ori2", "ord", "perc")  # the golden file's record
ALL_FIELDS = FIELDS + ("score", "mismatch_rate", "len0", "len1", "len2")
COUNTS = ("edges_before", "edges_after", "conflict_count", "n_moved", "n_switched", "tries", "best_try", "n_components", "n_inconsistent",
          "status", "bad_v", "bad_pos")


@functools.lru_cache(maxsize=None)
def load():
    with open(GOLDEN) as f:
        g = json.load(f)
    for c in g["cases"]:  # the input records are stored as rows
        c["edges"] = [dict(zip(g["edge_fields"], row)) for row in c["edges"]]
    return g


def golden_shuffles():
    """(lengths, {seed: SHA-256 of the seed's permutations as bytes, back to back in length order}, seed 1's bytes) of the golden file."""
    s = load()["shuffles"]
    seeds = range(s["seeds"][0], s["seeds"][1] + 1)
    return s["lengths"], dict(zip(seeds, s["sha256_by_seed"])), base64.b64decode(s["seed1_b64"])


def records(edges):
    """Full records of input edges (dicts v1, v2, ori1, ori2, pos1..pos4, ord) with the encoding of make_golden_labelling.py: read = vertex,
    perc = the record's index."""
    r = np.zeros(len(edges), EDGE_DTYPE)
    for k, e in enumerate(edges):
        for f in ("v1", "v2", "ori1", "ori2", "pos1", "pos2", "pos3", "pos4"):
            r[k][f] = e[f]
        r[k]["read1"], r[k]["read2"], r[k]["ord"], r[k]["perc"] = e["v1"], e["v2"], ord(e["ord"]), k
    r["score"], r["mismatch_rate"], r["len0"], r["len1"], r["len2"] = 1.0, 0.25, 30, 20, 10
    return r


def graph(V, edges):
    """(records, out_off, in_nodes, in_off) of the graph addEdge calls in the given order leave."""
    return _trans.csr_from_inserts(records(edges), V)


def golden_rows(recs):
    return [[int(r[f]) for f in FIELDS] for r in recs]


def same_graph(a, b):
    """(edges, out_off, in_nodes, in_off) equal array for array, every field of the records."""
    return all(np.array_equal(a[0][f], b[0][f]) for f in ALL_FIELDS) and all(
        np.array_equal(np.asarray(x, np.uint64), np.asarray(y, np.uint64)) for x, y in zip(a[1:], b[1:]))


def mirror(g, flags=2, n_reads=0):
    """The host mirror on a graph: ((edges, out_off, in_nodes, in_off), orientations, counts)."""
    V = len(g[1]) - 1
    m = _trans.Mirror(*g)
    fwd, counts = m.g.label_vertices(bool(flags & 2), bool(flags & 1), n_reads)
    edges, in_off, in_nodes = m.result()
    out_off = np.zeros(V + 1, np.uint64)
    np.add.at(out_off, edges["v1"].astype(np.int64) + 1, 1)
    return (edges, np.cumsum(out_off).astype(np.uint64), in_nodes.astype(np.uint32), in_off), fwd, counts


def random_edges(rng, V, n_edges, n_odd, n_components=1, paired=True):
    """Random simple digraph whose classes follow a hidden labelling, n_odd records against it; several components on request."""
    h = rng.integers(0, 2, V)
    comp = np.sort(rng.integers(0, n_components, V))
    seen, pairs = set(), []
    for v in range(1, V):
        if comp[v] == comp[v - 1]:
            lo = int(np.searchsorted(comp, comp[v]))
            u = int(rng.integers(lo, v))
            a, b = (u, v) if rng.random() < 0.5 else (v, u)
            seen.update(((a, b), (b, a)))
            pairs.append((a, b))
    tries = 0
    while len(pairs) < n_edges and tries < 50 * n_edges:
        tries += 1
        a, b = int(rng.integers(0, V)), int(rng.integers(0, V))
        if a == b or comp[a] != comp[b] or (a, b) in seen:
            continue
        seen.update(((a, b), (b, a)))
        pairs.append((a, b))
    rng.shuffle(pairs)
    odd = set(rng.choice(len(pairs), n_odd, replace=False).tolist()) if n_odd else set()
    out = []
    for k, (a, b) in enumerate(pairs):
        o1, o2 = int(h[a]), int(h[b])
        if rng.random() < 0.5:
            o1, o2 = 1 - o1, 1 - o2
        if k in odd:
            o2 = 1 - o2
        od = "-12"[int(rng.integers(0, 3))] if paired else "-"
        out.append(dict(v1=int(a), v2=int(b), ori1=o1, ori2=o2, pos1=int(rng.integers(0, 9)), pos2=int(rng.integers(0, 9)) if od != "-" else 0,
                        pos3=int(rng.choice((-3, -1, 0, 0, 2, 4))), pos4=int(rng.integers(-4, 5)) if od != "-" else 0, ord=od))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------

class Rand:
    """glibc srand / rand, TYPE_3."""

    def __init__(self, seed):
        word = seed if seed else 1
        r = [word]
        for _ in range(30):
            hi, lo = divmod(word, 127773)
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            r.append(word)
        self.r, self.f, self.b = r, 3, 0
        for _ in range(310):
            self.rand()

    def rand(self):
        self.r[self.f] = (self.r[self.f] + self.r[self.b]) & 0xFFFFFFFF
        x = self.r[self.f]
        self.f, self.b = (self.f + 1) % 31, (self.b + 1) % 31
        return x >> 1


def random_shuffle(seed, items):
    gen = Rand(seed)
    for i in range(1, len(items)):
        j = gen.rand() % (i + 1)
        if i != j:
            items[i], items[j] = items[j], items[i]


def switch_edge_orientation(e):
    e["pos1"], e["pos3"] = e["pos3"], e["pos1"]
    e["pos2"], e["pos4"] = e["pos4"], e["pos2"]
    e["ori1"], e["ori2"] = 1 - e["ori1"], 1 - e["ori2"]
    if e["pos1"] < 0 or (e["pos1"] == 0 and e["v1"] > e["v2"]):
        e["read1"], e["read2"] = e["read2"], e["read1"]
        e["v1"], e["v2"] = e["v2"], e["v1"]
        e["ori1"], e["ori2"] = e["ori2"], e["ori1"]
        e["pos1"] = -e["pos1"]
        if e["pos2"] < 0:
            e["ord"], e["pos2"] = ord("1"), -e["pos2"]
        elif e["ord"] != ord("-"):
            e["ord"] = ord("2")
        return True
    if e["pos2"] < 0:
        e["pos2"], e["ord"] = -e["pos2"], ord("2")
    elif e["ord"] != ord("-"):
        e["ord"] = ord("1")
    return False


class Restated:
    """vertexLabellingHeuristic restated over lists of dicts; rows() gives the records as the golden file lists them."""

    def __init__(self, g):
        edges, out_off, in_nodes, in_off = g
        self.V = len(out_off) - 1
        self.adj_out = [[{f: int(edges[k][f]) for f in FIELDS} for k in range(int(out_off[v]), int(out_off[v + 1]))] for v in range(self.V)]
        self.adj_in = [[int(x) for x in in_nodes[int(in_off[v]):int(in_off[v + 1])]] for v in range(self.V)]
        self.tries = self.conflict_count = 0

    def edge_info(self, v, w):
        for e in self.adj_out[v]:
            if e["v2"] == w:
                return e
        for e in self.adj_out[w]:
            if e["v2"] == v:
                return e
        raise AssertionError("Edge not found")

    def remove_with_ori(self, v, w, same):
        k = next(k for k, e in enumerate(self.adj_out[v]) if e["v2"] == w and (e["ori1"] == e["ori2"]) == same)
        del self.adj_out[v][k]
        if v in self.adj_in[w]:
            self.adj_in[w].remove(v)

    def label_vertices(self, orientations, seed):
        V = self.V
        orientations.extend([1] * (V - len(orientations)))
        visited = [False] * V
        moved, deleted = [], []
        for start in sorted(range(V), key=lambda v: (len(self.adj_in[v]), v)):
            bfs = []
            if not visited[start]:
                bfs.append(start)
                visited[start] = True
            head = 0
            while head < len(bfs):
                node = bfs[head]
                head += 1
                adj = list(self.adj_in[node]) + [e["v2"] for e in self.adj_out[node]]
                random_shuffle(seed, adj)
                for nb in adj:
                    if not visited[nb]:
                        bfs.append(nb)
                        visited[nb] = True
                        e = self.edge_info(node, nb)
                        orientations[nb] = orientations[node] if e["ori1"] == e["ori2"] else 1 - orientations[node]
        for lst in self.adj_out:
            for e in lst:
                t1, t2 = orientations[e["v1"]], orientations[e["v2"]]
                if e["ori1"] == t1 and e["ori2"] == t2:
                    continue
                if (e["ori1"] == e["ori2"]) != (t1 == t2):
                    deleted.append(dict(e))
                    continue
                c = dict(e)
                if switch_edge_orientation(c):
                    moved.append(c)
                else:
                    switch_edge_orientation(e)
        return moved, deleted

    def run(self):
        opt = [1] * self.V
        min_moved, min_deleted = self.label_vertices(opt, 1)
        orientations, count = [], 1
        while count < 100 and min_deleted:
            count += 1
            moved, deleted = self.label_vertices(orientations, count)
            if len(deleted) < len(min_deleted):
                min_moved, min_deleted, opt = moved, deleted, list(orientations)
        for e in min_moved:
            self.remove_with_ori(e["v2"], e["v1"], e["ori1"] == e["ori2"])
            self.adj_out[e["v1"]].append(e)
            self.adj_in[e["v2"]].append(e["v1"])
        for e in min_deleted:
            self.remove_with_ori(e["v1"], e["v2"], e["ori1"] == e["ori2"])
        self.tries, self.conflict_count = count, len(min_deleted)
        return opt

    def rows(self):
        return [[e[f] for f in FIELDS] for lst in self.adj_out for e in lst]

    def in_lists(self):
        return [x for lst in self.adj_in for x in lst]
