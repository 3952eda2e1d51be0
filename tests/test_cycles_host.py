"""OverlapGraph::sortEdges and cycleRemovalHeuristic on the host (hc_host_graph_sort_edges, hc_host_graph_remove_cycles,
hc_host_graph_find_cycles; no device): the mirror against the reference's own output on every case of tests/golden/cycles.json — the
lists after sortEdges, all 20 per-try sets, both lists, branching_edges, backedge_count and cycles.txt for both values of remove_edges;
the iterative walk on a 200 000-vertex chain, open and closed into a ring; the permutation tables against the hashes recorded in
tests/golden/labelling.json; the statuses."""
import hashlib

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import cycles as CY
from tests import _cycles as Y
from tests import _labelling as L

CASES = Y.load()["cases"]
IDS = [c["name"] for c in CASES]


def sorted_graph(case):
    recs = Y.case_records(case["edges"])
    return Y.host_sorted(Y.inserted(case["V"], recs), np.asarray(case["len_by_read"], np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sort_edges_equals_the_reference(case):
    edges, out_off, in_nodes, in_off = sorted_graph(case)
    assert edges["perc"].tolist() == case["sorted_out"] and out_off.tolist() == case["sorted_out_off"]
    assert in_nodes.tolist() == case["sorted_in"] and in_off.tolist() == case["sorted_in_off"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_try_equals_the_reference(case):
    edges, out_off, _, in_off = sorted_graph(case)
    for t in range(1, 21):
        assert CY.host_find_cycles(edges, out_off, in_off, t).tolist() == case["sets"][t - 1], t


@pytest.mark.parametrize("remove", [True, False], ids=["remove", "keep"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mirror_equals_the_reference(case, remove):
    g = sorted_graph(case)
    want = case["remove" if remove else "keep"]
    r = Y.mirror(g, remove)
    assert r.edges["perc"].tolist() == want["out"] and r.out_off.tolist() == want["out_off"]
    assert r.in_nodes.tolist() == want["in_nodes"] and r.in_off.tolist() == want["in_off"]
    assert r.removed["perc"].tolist() == want["branching"]
    assert r.counts["backedge_count"] == want["backedge_count"] and r.counts["status"] == 0
    txt = r.cycles_txt()
    assert (txt.decode() if txt is not None else None) == want["cycles_txt"]
    sizes = [len(s) for s in case["sets"]]
    if sizes[0] == 0:
        assert (r.counts["tries"], r.counts["best_try"], r.counts["try_size"]) == (1, 1, [0] * 20)
    else:
        assert (r.counts["tries"], r.counts["best_try"], r.counts["try_size"]) == (20, sizes.index(min(sizes)) + 1, sizes)
    assert r.counts["edges_before"] == len(case["edges"]) and r.counts["edges_after"] == len(want["out"])
    # the records travel untouched
    recs = Y.case_records(case["edges"])
    assert Y.same_records(r.edges, recs[r.edges["perc"]]) and Y.same_records(r.removed, recs[r.removed["perc"]])


def test_flagged_components_are_counted():
    by = {c["name"]: c for c in CASES}
    c = Y.mirror(sorted_graph(by["two_cyclic_among_acyclic"])).counts
    assert (c["n_flagged_components"], c["n_host_vertices"]) == (2, 4 + 7)
    c = Y.mirror(sorted_graph(by["acyclic"])).counts
    assert (c["n_flagged_components"], c["n_host_vertices"], c["n_host_edges"]) == (0, 0, 0)


@pytest.mark.parametrize("closed", [False, True], ids=["chain", "ring"])
def test_walk_is_iterative_on_a_long_path(closed):
    V = 200000
    recs, lens = Y.chain(V, closed)
    g = Y.inserted(V, recs)  # one record per list: every order is sortEdges'
    pairs = CY.host_find_cycles(g[0], g[1], g[3], 1)
    # the ring: every in-degree is 1, so the walk starts at 0 and closes at V - 1 -> 0
    assert pairs.tolist() == ([[V - 1, 0]] if closed else [])
    r = Y.mirror(g, True, n_threads=4)
    assert r.counts["backedge_count"] == int(closed) and r.counts["tries"] == (20 if closed else 1)
    assert r.counts["try_size"] == [int(closed)] * 20 and r.edges.shape[0] == recs.shape[0] - int(closed)
    assert r.pairs.tolist() == pairs.tolist()


def test_threads_do_not_change_the_result():
    rng = np.random.default_rng(3)
    V = 400
    recs = Y.random_records(rng, V, 1500)
    g = Y.host_sorted(Y.inserted(V, recs), rng.integers(60, 140, V).astype(np.uint32))
    a, b = Y.mirror(g, True, 1), Y.mirror(g, True, 7)
    assert a.counts == b.counts and a.counts["tries"] == 20 and a.pairs.tolist() == b.pairs.tolist()
    assert Y.same_graph(Y.graph_of(a), Y.graph_of(b)) and Y.same_records(a.removed, b.removed)
    # one record per pair left, in the pairs' order
    assert np.array_equal(a.removed["v1"], a.pairs[:, 0]) and np.array_equal(a.removed["v2"], a.pairs[:, 1])
    assert a.edges.shape[0] == g[0].shape[0] - a.pairs.shape[0]


def test_permutation_tables_equal_the_recorded_shuffles():
    lengths, digests, _ = L.golden_shuffles()
    tables = {n: CY.perm_table(n) for n in lengths}
    for t in range(5, 21):
        got = b"".join(bytes(tables[n][t - 5].astype(np.uint8)) for n in lengths)
        assert hashlib.sha256(got).hexdigest() == digests[t], t
    assert CY.perm_table(0).shape == (16, 0) and CY.perm_table(1).tolist() == [[0]] * 16


def test_nan_key_is_refused_untouched():
    recs = Y.records([0, 1, 2, 3], [1, 2, 0, 4], score=[1.0, 1.0, 1.0, float("nan")])
    g = Y.inserted(5, recs)
    r = Y.mirror(g)
    assert (r.status, r.counts["bad_v"], r.counts["bad_pos"]) == ("NAN_KEY", 3, 0)
    assert Y.same_graph(Y.graph_of(r), g) and r.pairs.shape[0] == 0 and r.removed.shape[0] == 0
    # without a cycle the other tries never run, and the reference never compares the value
    recs = Y.records([0, 1, 3], [1, 2, 4], mismatch_rate=[0.25, 0.25, float("nan")])
    r = Y.mirror(Y.inserted(5, recs))
    assert r.status == "OK" and r.counts["tries"] == 1


def test_more_pairs_than_room_is_an_error():
    import ctypes as C

    recs = Y.records([0, 1, 2, 3], [1, 0, 3, 2])
    e, oo, inn, io = Y.inserted(4, recs)
    st, c = CY.hc_cycles_settings(1, 0), CY.hc_cycles_counts()
    pairs = np.zeros((1, 2), np.uint32)
    rc = N.lib.hc_host_graph_remove_cycles(e.ctypes.data, oo.ctypes.data, inn.ctypes.data, io.ctypes.data, 4, C.byref(st), 1, None, None, None, None, None,
                                           pairs.ctypes.data, 1, C.byref(c))
    assert rc != 0 and c.backedge_count == 2
