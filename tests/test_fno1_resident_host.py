"""hc_host_fno1_walk_edges (include/hcsr.h) — the edge list host/FindNextOverlaps.cpp walks — against a Python restatement of reference
src/FindNextOverlaps.cpp:612-630, :694 and :816-887 (tests/_fno1_resident.py): the reference's golden runs, seeded scenarios that hold every
vertex relation of :841-865, a group with paired reads, induced pairs whose edge exists forward, reversed only or with score 0, and a
read shorter than pos1.  The returned list, fed back to hc_fno1_run as plain graph_edges, reproduces the text.  No GPU."""
import numpy as np
import pytest

from haploconduct_amd import HcError
from haploconduct_amd import fno as F
from tests import _fno as T
from tests import _fno1_resident as R


@pytest.fixture(autouse=True)
def _host_threads(monkeypatch):
    monkeypatch.setenv("HC_FNO", "host")


def _check(inp, what, want_text=None):
    want, want_seg = R.restated_walk_edges(inp)
    got, seg = F.host_walk_edges(inp)
    assert seg == want_seg, (what, seg, want_seg)
    R.same_edges(got, want, what)
    text, counters = F.find_next_overlaps(inp)
    if want_text is not None:
        assert text == want_text, what
    text2, counters2 = F.find_next_overlaps(R.as_graph_edges_only(inp, got))
    assert text2 == text and counters2 == counters, what
    return got, seg


def test_the_references_golden_runs():
    n, induced, kept, dropped = 0, 0, 0, 0
    for name, inp, want_text in R.golden_inputs():
        _, seg = _check(inp, name, want_text)
        n += 1
        induced += seg[3]
        kept += seg[2]
        dropped += len(inp.nonedges) - seg[2] if not inp.flags & F.OPTIMIZE else 0
    assert n == 18 and induced > 0 and kept > 0 and dropped > 0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("flags", [F.RESOLVE_ORIENTATIONS, F.RESOLVE_ORIENTATIONS | F.OPTIMIZE, F.NO_INCLUSIONS])
def test_seeded_scenarios_with_every_source(seed, flags):
    inp = T.fno1_scenario(seed, n_nodes=60, n_srs=16, n_edges=300, with_extras=True, flags=flags)
    _, seg = _check(inp, f"seed {seed} flags {flags}")
    assert seg[0] == 300 and seg[1] == 50 and seg[3] > 0
    assert (seg[2] == 0) == bool(flags & F.OPTIMIZE)


def _star(w, outs, ins, pos=5):
    """the group of inclusion vertex w: its out-edges, then its in-edges"""
    return np.array([T.make_edge(w, x, pos + k, perc=100) for k, x in enumerate(outs)] + [T.make_edge(y, w, pos + 10 + k, perc=100) for k, y in enumerate(ins)],
                    F.FNO_EDGE_DTYPE)


def _hand(nodes_spec, graph, groups, nonedges=None, threshold=0.97):
    nodes = np.zeros(len(nodes_spec), F.FNO_READ_DTYPE)
    for u, (l1, l2, p) in enumerate(nodes_spec):
        nodes[u] = T.make_read(u, l1, l2, p)
    ge = np.array(graph, F.FNO_EDGE_DTYPE) if graph else np.zeros(0, F.FNO_EDGE_DTYPE)
    ge = ge[np.argsort(ge["v1"], kind="stable")]
    return F.Fno1Input(nodes, np.zeros(0, F.FNO_READ_DTYPE), [], [], ge, inclusion_groups=groups, nonedges=nonedges, new_read_count=len(nodes),
                       edge_threshold=threshold)


def test_every_vertex_relation_of_841_865():
    """w = 0 with out-edges to 1, 2 and in-edges from 3, 4, in both orders of (edge1, edge2): same source (skipped), edge1's source is
    edge2's target, edge1's target is edge2's source, same target (skipped)"""
    nodes = [(100, 0, 0)] * 5
    fwd = _star(0, [1, 2], [3, 4])
    inp = _hand(nodes, [], [fwd, fwd[::-1].copy(), fwd[[2, 0, 3, 1]].copy()])
    got, seg = _check(inp, "relations")
    assert seg == [0, 0, 0, 12]  # 4 of the 6 pairs of every group induce y -> x
    assert {(int(e["v1"]), int(e["v2"])) for e in got} == {(3, 1), (3, 2), (4, 1), (4, 2)}
    # pos1 and ori1 come from the in-edge (the head), ori2 from the out-edge (the tail)
    first = got[0]
    assert (int(first["v1"]), int(first["v2"]), int(first["pos1"]), int(first["len1"]), int(first["perc"])) == (3, 1, 15, 85, 85)


def test_a_group_with_paired_reads_skips_their_pairs():
    nodes = [(100, 0, 0), (100, 0, 0), (100, 80, 1), (100, 0, 0), (90, 70, 1)]
    inp = _hand(nodes, [], [_star(0, [1, 2], [3, 4])])
    got, seg = _check(inp, "paired reads")
    assert seg[3] == 1 and (int(got[0]["v1"]), int(got[0]["v2"])) == (3, 1)


def test_the_induced_edge_exists_forward_reversed_only_or_with_score_0():
    nodes = [(100, 0, 0)] * 8
    graph = [T.make_edge(4, 1, 3, score=0.99),   # y -> x exists forward
             T.make_edge(2, 5, 3, score=0.99),   # x -> y only: checkEdge looks at the reverse list too
             T.make_edge(6, 3, 3, score=0.0),    # exists with score 0: an edge for :876 (== -1 fails), none for :694 (> 0 fails)
             T.make_edge(7, 1, 9, score=0.5), T.make_edge(1, 7, 9, score=0.0)]  # forward first: the score is the forward record's
    ne = np.array([T.make_edge(6, 3, 2, score=0.0), T.make_edge(3, 6, 2, score=0.0), T.make_edge(4, 1, 2, score=0.0), T.make_edge(1, 7, 2, score=0.0),
                   T.make_edge(0, 5, 2, score=0.0)], F.FNO_EDGE_DTYPE)
    inp = _hand(nodes, graph, [_star(0, [1, 2, 3], [4, 5, 6, 7])], nonedges=ne)
    got, seg = _check(inp, "existing edges")
    induced = {(int(e["v1"]), int(e["v2"])) for e in got[sum(seg[:3]):]}
    assert induced == {(y, x) for y in (4, 5, 6, 7) for x in (1, 2, 3)} - {(4, 1), (5, 2), (6, 3), (7, 1)}
    kept = [(int(e["v1"]), int(e["v2"])) for e in got[sum(seg[:2]):sum(seg[:3])]]
    assert kept == [(6, 3), (3, 6), (1, 7), (0, 5)]  # (1, 7): its own list says score 0 first; (4, 1) sits behind 0.99


def test_a_read_shorter_than_pos1():
    """len1 - pos1 is unsigned in the reference: it wraps, and the minimum is the other read's length"""
    nodes = [(100, 0, 0), (60, 0, 0), (100, 0, 0), (20, 0, 0)]
    grp = np.array([T.make_edge(0, 1, 5, perc=100), T.make_edge(3, 0, 45, perc=100)], F.FNO_EDGE_DTYPE)  # head 3 -> 0 at pos1 45 > len 20
    got, seg = _check(_hand(nodes, [], [grp]), "wrap")
    assert seg[3] == 1 and (int(got[0]["len1"]), int(got[0]["perc"]), int(got[0]["pos1"])) == (60, 300, 45)


def test_where_the_reference_stops_and_what_is_refused():
    nodes = [(100, 0, 0)] * 5
    bad = np.array([T.make_edge(0, 1, 5), T.make_edge(2, 3, 5)], F.FNO_EDGE_DTYPE)  # no vertex in common: the assert of :863
    with pytest.raises(HcError) as e:
        F.host_walk_edges(_hand(nodes, [], [bad]))
    assert e.value.status == -9  # HC_ERR_FORMAT
    with pytest.raises(R.RefStop):
        R.restated_walk_edges(_hand(nodes, [], [bad]))
    inp = T.fno1_scenario(5, n_nodes=40, with_extras=True, dup=True, flags=F.ADD_DUPLICATES)
    with pytest.raises(HcError) as e:
        F.host_walk_edges(inp)
    assert e.value.status == -1  # HC_ERR_ARG: hc_fno1_run's
    # count, then fetch: a buffer one record short is refused with the sizes filled
    import ctypes as C
    from haploconduct_amd import _native as N
    inp = T.fno1_scenario(6, with_extras=True)
    s, seg = inp.struct(), (C.c_uint64 * 4)()
    n = len(F.host_walk_edges(inp)[0])
    buf = np.zeros(n, F.FNO_EDGE_DTYPE)
    assert N.lib.hc_host_fno1_walk_edges(C.byref(s), buf.ctypes.data, n - 1, C.byref(seg)) == -1 and sum(seg) == n and not buf["v1"].any()
