"""Shared by the hc_fno1_from_graph tests: a Python restatement of how SRBuilder::findNextOverlaps collects the edges it walks (reference
src/FindNextOverlaps.cpp:612-630 adj_out and branching_edges, :694 the stored non-edges behind checkEdge, :816-887 the inclusion-induced
edges, src/OverlapGraph.cpp:233-259 checkEdge itself), the golden scenarios as Fno1Input, and seeded builders: super-read tables over the
vertices of a graph, graph records whose columns agree with those tables, stored non-edges of which a part sits behind an edge."""
import json
import os

import numpy as np

from haploconduct_amd import fno as F
from haploconduct_amd.host import EDGE_DTYPE
from tests import _fno as T
from tests import _trans

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fno")
ECOLS = ["v1", "v2", "score", "pos1", "pos2", "len1", "len2", "perc", "ord", "ori1", "ori2"]
EDGE_FIELDS = ECOLS + ["pad"]


def _rec(rows, dtype, names):
    a = np.zeros(len(rows), dtype)
    for k, name in enumerate(names):
        a[name] = [r[k] for r in rows]
    return a


def golden_inputs():
    """(name, Fno1Input, expected text) for every case of fno1_run.json and fno1_run_nonedges.json (the reference's own runs)."""
    from haploconduct_amd import host
    from haploconduct_amd.records import OVERLAP_DTYPE

    for fname in ("fno1_run.json", "fno1_run_nonedges.json"):
        g = json.load(open(os.path.join(GOLD, fname)))
        for k, c in enumerate(g["cases"]):
            nodes = _rec(c["nodes"], F.FNO_READ_DTYPE, ["id", "len1", "len2", "paired", "visited", "orientation"])
            srs = _rec(c["srs"], F.FNO_READ_DTYPE, ["id", "len1", "len2", "paired"])
            subs = _rec(c["subreads"], F.FNO_SUBREAD_DTYPE, ["node", "index1", "index2", "startpos1", "startpos2"])
            co, so, io = c["clique_off"], c["subread_off"], c["inclusion_off"]
            cliques = [np.array(c["clique_nodes"][co[i]:co[i + 1]], np.uint64) for i in range(len(srs))]
            subreads = [subs[so[i]:so[i + 1]] for i in range(len(srs))]
            incl = _rec(c["inclusion_edges"], F.FNO_EDGE_DTYPE, ECOLS)
            groups = [incl[io[i]:io[i + 1]] for i in range(len(io) - 1)]
            nonedges = None
            if "nonedge_lines" in c:
                recs = np.zeros(len(c["nonedge_lines"]), OVERLAP_DTYPE)
                for j, ln in enumerate(c["nonedge_lines"]):
                    rc, o = host.parse_overlap(ln)
                    assert rc == 0
                    recs[j] = (o["id1"], o["id2"], o["pos1"], o["pos2"], o["ori1"] == "+", o["ori2"] == "+", ord(o["ord"]), 0, o["len1"], o["len2"], o["perc"])
                nonedges = F.edges_from_records(recs)
            inp = F.Fno1Input(nodes, srs, cliques, subreads, _rec(c["graph_edges"], F.FNO_EDGE_DTYPE, ECOLS),
                              branching_edges=_rec(c["branching_edges"], F.FNO_EDGE_DTYPE, ECOLS), nonedges=nonedges, inclusion_groups=groups,
                              new_read_count=c["new_read_count"], edge_threshold=c["edge_threshold"], flags=c["flags"])
            yield f"{fname}[{k}]", inp, c["text"].encode()


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
class RefStop(Exception):
    """the reference would assert here"""


def adjacency(inp):
    """OverlapGraph::adj_out: per vertex the (v2, score) of its edges in list order"""
    adj = [[] for _ in range(len(inp.nodes))]
    for e in inp.graph_edges:
        adj[int(e["v1"])].append((int(e["v2"]), float(e["score"])))
    return adj


def check_edge(adj, v, w):
    """OverlapGraph::checkEdge(v, w, true), src/OverlapGraph.cpp:233-259: the first v -> w in v's list, else the first w -> v in w's, else -1"""
    for v2, score in adj[v]:
        if v2 == w:
            return score
    for v2, score in adj[w]:
        if v2 == v:
            return score
    return -1.0


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def induced_edge(e1, e2, nodes, edge_threshold):
    """:841-875 for edge1 = e1, edge2 = e2: None where the pair induces nothing, else the new Edge as a FNO_EDGE_DTYPE record"""
    if e1["v1"] == e2["v1"]:
        return None
    if e1["v1"] == e2["v2"]:
        head, tail = e2, e1
    elif e1["v2"] == e2["v1"]:
        head, tail = e1, e2
    else:
        if e1["v2"] != e2["v2"]:
            raise RefStop("assert (edge1.get_vertex(2) == edge2.get_vertex(2))")
        return None
    r1, r2 = nodes[int(head["v1"])], nodes[int(tail["v2"])]
    if r1["paired"] or r2["paired"]:
        return None
    l1, l2 = int(r1["len1"]), int(r2["len1"])
    ln = _i32(min((l1 - int(head["pos1"])) & 0xFFFFFFFF, l2))  # unsigned get_len() - int pos1, the minimum assigned to an int
    if min(l1, l2) == 0:
        raise RefStop("division by zero")
    perc = _i32(((100 * ln) & 0xFFFFFFFF) // min(l1, l2))
    if ln <= 0:
        raise RefStop("Edge::set_len")
    return T.make_edge(int(head["v1"]), int(tail["v2"]), int(head["pos1"]), 0, "-", score=edge_threshold, len1=ln, len2=0, perc=perc,
                       ori1=int(head["ori1"]), ori2=int(tail["ori2"]))


def restated_walk_edges(inp):
    """The edges updateOverlap is called on, in order -> (FNO_EDGE_DTYPE array, [the four segment lengths])."""
    adj = adjacency(inp)
    seg = [list(inp.graph_edges), list(inp.branching_edges), [], []]  # :612-624 (graph_edges come vertex by vertex), :627-630
    if not inp.flags & F.OPTIMIZE:  # :926
        seg[2] = [e for e in inp.nonedges if not check_edge(adj, int(e["v1"]), int(e["v2"])) > 0]  # :694
    for g in range(inp.n_inclusion_groups):  # :822-881
        grp = inp.inclusion_edges[int(inp.inclusion_off[g]):int(inp.inclusion_off[g + 1])]
        for i in range(len(grp)):
            for j in range(i + 1, len(grp)):
                ne = induced_edge(grp[i], grp[j], inp.nodes, inp.edge_threshold)
                if ne is not None and check_edge(adj, int(ne["v1"]), int(ne["v2"])) == -1:
                    seg[3].append(ne)
    flat = [e for s in seg for e in s]
    return (np.array(flat, F.FNO_EDGE_DTYPE) if flat else np.zeros(0, F.FNO_EDGE_DTYPE)), [len(s) for s in seg]


def same_edges(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in EDGE_FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, int(bad[0]), got[int(bad[0])], want[int(bad[0])])


def as_graph_edges_only(inp, edges):
    """The same tables with `edges` as plain graph_edges and no other source: hc_fno1_run walks exactly that list."""
    import copy

    out = copy.copy(inp)
    e0 = np.zeros(0, F.FNO_EDGE_DTYPE)
    out.graph_edges, out.branching_edges, out.nonedges = np.ascontiguousarray(edges), e0, e0
    out.inclusion_off, out.inclusion_edges, out.n_inclusion_groups = np.zeros(1, np.uint64), e0, 0
    return out


# ---- seeded builders ----------------------------------------------------------------------------------------------------------------------
def seeded_tables(seed, V, n_srs, paired_frac=0.3, clique=(2, 7)):
    """Vertex and super-read tables over V vertices as _fno.fno1_scenario draws them: every precondition the reference asserts holds.
    -> (nodes, srs, clique_off, clique_nodes, subread_off, subreads, new_read_count)"""
    rng = np.random.default_rng(seed)
    paired = rng.random(V) < paired_frac
    cliques, sr_paired = [], []
    for _ in range(n_srs):
        p = bool(rng.random() < paired_frac) and paired.sum() >= clique[1]
        pool = np.flatnonzero(paired) if p else np.arange(V)
        cliques.append(rng.choice(pool, size=int(rng.integers(*clique)), replace=False).astype(np.uint64))
        sr_paired.append(p)
    order = sorted(range(n_srs), key=lambda i: sr_paired[i])  # single_SR_vec before paired_SR_vec
    cliques, sr_paired = [cliques[i] for i in order], [sr_paired[i] for i in order]
    visited = np.zeros(V, bool)
    for c in cliques:
        visited[c.astype(int)] = True
    visited |= rng.random(V) < 0.03
    nodes = np.zeros(V, F.FNO_READ_DTYPE)
    nodes["len1"], nodes["len2"] = rng.integers(40, 300, V) | 1, np.where(paired, rng.integers(40, 300, V), 0)  # odd: see graph_records
    nodes["paired"], nodes["visited"], nodes["orientation"] = paired, visited, rng.integers(0, 2, V)
    nodes["id"][~visited] = np.arange(int((~visited).sum()))
    next_id = int((~visited).sum())
    srs = np.zeros(n_srs, F.FNO_READ_DTYPE)
    srs["id"] = next_id + np.arange(n_srs)
    srs["len1"], srs["paired"] = rng.integers(100, 900, n_srs), sr_paired
    srs["len2"] = np.where(srs["paired"] != 0, rng.integers(100, 900, n_srs), 0)
    subreads = []
    for c in cliques:
        sub = np.zeros(len(c), F.FNO_SUBREAD_DTYPE)
        sub["node"] = c
        for a, b in (("index1", "startpos1"), ("index2", "startpos2")):
            trimmed = rng.random(len(c)) < 0.3
            sub[b] = np.where(trimmed, rng.integers(0, 60, len(c)), 0)
            sub[a] = np.where(trimmed, 0, rng.integers(0, 500, len(c)))
        subreads.append(sub[rng.permutation(len(sub))])  # any order inside a super-read
    co, cn = F._csr(cliques, np.uint64)
    so, sub = F._csr(subreads, F.FNO_SUBREAD_DTYPE)
    return nodes, srs, co, cn, so, sub, next_id + n_srs


def agree_with_nodes(recs, nodes, seed):
    """Graph records (EDGE_DTYPE or FNO_EDGE_DTYPE) whose ord / pos2 / len2 / perc agree with the vertices' types, as the Edge constructor
    and updateOverlap's asserts want them; len1 > 0."""
    rng = np.random.default_rng(seed)
    n = len(recs)
    p1, p2 = nodes["paired"][recs["v1"].astype(np.int64)] != 0, nodes["paired"][recs["v2"].astype(np.int64)] != 0
    recs["ord"] = np.where(p1 & p2, rng.choice([ord("1"), ord("2")], n), ord("-"))
    recs["pos2"] = np.where(p1 | p2, rng.integers(0, 260, n), 0)
    recs["len2"] = np.where(p1 | p2, rng.integers(0, 300, n), 0)
    recs["len1"] = np.maximum(recs["len1"], 1)
    recs["perc"] = np.where(rng.random(n) < 0.1, 100, rng.integers(0, 100, n))
    recs["ori1"], recs["ori2"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
    return recs


def graph_records(v1, v2, nodes, seed, scores=(0.5, 0.98, 1.0)):
    """EDGE_DTYPE records for the edges (v1[i], v2[i]) in insertion order, columns in agreement with `nodes`.  pos1 is even and
    seeded_tables' lengths are odd: a read may be shorter than pos1 (the induced length wraps, :870) but never exactly as long (Edge::set_len
    would stop the reference at a length of 0)."""
    rng = np.random.default_rng(seed)
    r = _trans.make_records(np.asarray(v1), np.asarray(v2), seed)
    r["score"] = rng.choice(list(scores), len(r))
    r["pos1"] = 2 * rng.integers(0, 130, len(r))
    return agree_with_nodes(r, nodes, seed + 1)


def seeded_nonedges(seed, n, nodes, graph_edges, behind_frac=1 / 3):
    """n stored non-edges (score 0) over the vertices; the first behind_frac of them between vertices an edge of the graph joins, in either
    direction (checkEdge > 0 drops those whose edge has a positive score), then shuffled."""
    rng = np.random.default_rng(seed)
    V = len(nodes)
    ne = np.zeros(n, F.FNO_EDGE_DTYPE)
    ne["v1"] = rng.integers(0, V, n)
    ne["v2"] = (ne["v1"] + rng.integers(1, V, n)) % V
    k = int(n * behind_frac)
    if k and len(graph_edges):
        pick = graph_edges[rng.integers(0, len(graph_edges), k)]
        flip = rng.random(k) < 0.5
        ne["v1"][:k] = np.where(flip, pick["v2"], pick["v1"])
        ne["v2"][:k] = np.where(flip, pick["v1"], pick["v2"])
    ne["pos1"], ne["len1"] = rng.integers(0, 260, n), rng.integers(1, 300, n)
    ne = agree_with_nodes(ne, nodes, seed + 1)
    return ne[rng.permutation(n)]


def load(sc, recs, V, inclusions=None):
    """hc_graph_load of the records in insertion order"""
    edges, out_off, in_nodes, in_off = _trans.csr_from_inserts(recs, V)
    sc.graph_load(edges, out_off, in_nodes, in_off, inclusions)
    return edges


def expected(sc, tables, nonedges=None, **kw):
    """hc_fno1_run on the host threads (HC_FNO=host) for what the context holds, through the three fetches -> (inp, text, counters)"""
    inp = F.input_from_context(sc, tables, nonedges, **kw)
    old = os.environ.get("HC_FNO")
    os.environ["HC_FNO"] = "host"
    try:
        text, counters = F.find_next_overlaps(inp)
        assert not F.last_on_device
    finally:
        if old is None:
            os.environ.pop("HC_FNO", None)
        else:
            os.environ["HC_FNO"] = old
    return inp, text, counters


def assert_same_run(sc, res, inp, text, counters, what=""):
    """the device's edge list per segment against the host helper's, then the text and the four counters"""
    want_edges, want_seg = F.host_walk_edges(inp)
    got_edges, got_seg = sc.fno1_edges()
    assert got_seg == want_seg, (what, got_seg, want_seg)
    at = 0
    for k, n in enumerate(want_seg):
        same_edges(got_edges[at:at + n], want_edges[at:at + n], f"{what} segment {k}")
        at += n
    got_text = sc.fno1_text()
    assert got_text == text, (what, len(got_text), len(text))
    c = res.counts
    assert {k: c[k] for k in ("n_lines", "copied", "u2sr", "v2sr", "sr2sr")} == {k: counters[k] for k in ("n_lines", "copied", "u2sr", "v2sr", "sr2sr")}, what
    assert c["n_bytes"] == len(text) and c["n_lines"] == text.count(b"\n"), what
