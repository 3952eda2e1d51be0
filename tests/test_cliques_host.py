"""The host mirror of hc_graph_cliques (hc_host_graph_cliques) against quick-cliques' own output (tests/golden/cliques.json, made by
tests/golden/make_golden_cliques.py) as sets, against an exhaustive subset check on small graphs, and against the Python restatement
of the order rule (tests/_cliques.py) array for array; the pair set's independence of how the records carry it, the two asserts, the
budget and count-then-fetch."""
import ctypes as C

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import cliques as CL
from haploconduct_amd.clique_next import host_clique_select
from tests import _cliques as K
from tests import _graph_text as GT

CASES = K.load_cases()
HC_ERR_ARG = -1


def mirror(g, **kw):
    edges, out_off, _, _, incl = g
    return CL.host_graph_cliques(edges, out_off, incl, **kw)


def as_lists(c):
    return [[int(x) for x in c.row(k)] for k in range(c.clique_off.size - 1)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_equals_quick_cliques_as_sets(case):
    want, text = K.qc_cliques(case["qc_stdout"])
    got = mirror(K.case_graph(case))
    assert got.status == "OK"
    assert got.as_set() == set(want) and got.counts["n_cliques"] == len(want), case["name"]
    c = got.counts
    assert c["n_entries"] == sum(map(len, want)) == got.clique_nodes.size
    assert c["n_singletons"] == sum(len(x) == 1 for x in want) and c["max_clique"] == max(map(len, want))
    assert c["n_pairs"] == len(K.pair_set(case["n_vertices"], case["edges"], case["inclusions"]))
    assert len(text) == 2  # the reference's logged clique_count is n_cliques + 2 (src/SRBuilder.cpp:1057)


def test_golden_covers_what_the_issue_lists():
    by = {c["name"]: K.qc_cliques(c["qc_stdout"])[0] for c in CASES}
    assert {n[5:] for n in by if n.startswith("file_")} == {c["name"] for c in GT.load_cases()}  # every graph.txt of graph_files.json
    assert len(by["moon_moser_5x3"]) == 245 and sum(map(len, by["moon_moser_5x3"])) == 1217
    for n in (63, 64, 65, 129):
        assert sorted(map(len, by[f"k{n}"])) == [1, n]
    assert len(by["hub_65_triangles"]) == 65
    # the random graphs, as the golden script's seeds give them (it holds the same figures): cliques, largest clique
    pinned = {"interval_300": (226, 13), "interval_2000": (1542, 15), "gnp_40_0": (418, 7), "gnp_40_1": (427, 6), "gnp_40_2": (460, 6)}
    assert {n: (len(by[n]), max(map(len, by[n]))) for n in pinned} == pinned
    assert all(400 <= pinned[f"gnp_40_{k}"][0] <= 520 for k in range(3))
    # a graph.txt with a pair on several lines is not a graph qc enumerates: what it did with the file as written is on record
    repeated = [c for c in CASES if c.get("repeated_lines")]
    assert repeated and any(c["qc_exit_as_written"] != 0 for c in repeated)
    assert any(c["qc_exit_as_written"] == 0 and set(K.qc_cliques(c["qc_stdout_as_written"])[0]) != set(K.qc_cliques(c["qc_stdout"])[0]) for c in repeated)


def small_family():
    rng = np.random.default_rng(14)
    for n in list(range(1, 15)) + [14, 14, 13, 12]:
        for p in (0.0, 0.2, 0.5, 0.8, 1.0):
            yield n, [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < p]


def test_mirror_equals_exhaustive_enumeration():
    for n, pairs in small_family():
        got = mirror(K.graph(n, pairs))
        assert got.as_set() == K.exhaustive(n, pairs) and got.counts["n_cliques"] == len(got.as_set()), (n, pairs)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_equals_the_restated_rule(case):
    got = mirror(K.case_graph(case))
    want = K.restate(case["n_vertices"], K.pair_set(case["n_vertices"], case["edges"], case["inclusions"]))
    off, nodes = K.csr(want)
    assert np.array_equal(got.clique_off, off) and np.array_equal(got.clique_nodes, nodes), case["name"]


def test_small_family_in_rule_order_and_threads():
    for n, pairs in small_family():
        off, nodes = K.csr(K.restate(n, pairs))
        for nt in (1, 4):
            got = mirror(K.graph(n, pairs), n_threads=nt)
            assert np.array_equal(got.clique_off, off) and np.array_equal(got.clique_nodes, nodes), (n, pairs, nt)


def test_pairs_one_way_both_ways_and_repeated():
    case = next(c for c in CASES if c["name"] == "gnp_40_0")
    V, pairs = case["n_vertices"], [tuple(e) for e in case["edges"]]
    one = mirror(K.graph(V, pairs))
    rng = np.random.default_rng(3)
    forms = {"flipped": [(b, a) for a, b in pairs], "both": pairs + [(b, a) for a, b in pairs],
             "repeated": [pairs[i] for i in rng.integers(0, len(pairs), 3 * len(pairs))] + pairs + [(b, a) for a, b in pairs[::3]]}
    for name, form in forms.items():
        form = [form[i] for i in rng.permutation(len(form))]
        got = mirror(K.graph(V, form, seed=5))
        assert np.array_equal(got.clique_off, one.clique_off) and np.array_equal(got.clique_nodes, one.clique_nodes), name
        assert got.counts["n_pairs"] == one.counts["n_pairs"] == len(pairs)


def test_inclusion_endpoints_are_dropped():
    # 0-1-2 a triangle, 3 an inclusion vertex everything points at: its records give no pair, and it is a clique of one
    pairs = [(0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3), (4, 3)]
    got = mirror(K.graph(6, pairs, incl=[0, 0, 0, 1, 0, 0]))
    assert got.status == "OK" and got.as_set() == {(0, 1, 2), (3,), (4,), (5,)}
    assert got.counts["n_pairs"] == 3 and got.counts["n_singletons"] == 3
    assert as_lists(got) == K.restate(6, K.pair_set(6, pairs, [0, 0, 0, 1, 0, 0]))


def test_assert_statuses_first_in_file_order():
    got = mirror(K.graph(6, [(0, 1), (2, 3), (2, 2), (4, 4), (2, 5)]))
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("SELF_LOOP", 2, 1)
    assert got.counts["n_cliques"] == 0 and got.clique_nodes.size == 0
    got = mirror(K.graph(6, [(0, 1), (3, 4), (3, 5), (5, 0)], incl=[0, 0, 0, 1, 0, 1]))
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("INCLUSION_HAS_EDGES", 3, 0)
    # the earlier place wins whichever assert it is; a self-loop behind an inclusion target is still one
    got = mirror(K.graph(6, [(1, 1), (3, 4)], incl=[0, 0, 0, 1, 0, 0]))
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("SELF_LOOP", 1, 0)
    got = mirror(K.graph(6, [(1, 3), (1, 1), (3, 4)], incl=[0, 0, 0, 1, 0, 0]))
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("SELF_LOOP", 1, 1)
    got = mirror(K.graph(6, [(1, 0), (4, 4)], incl=[0, 1, 0, 0, 0, 0]))
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("INCLUSION_HAS_EDGES", 1, 0)


@pytest.mark.parametrize("name", ["moon_moser_5x3", "interval_300", "file_edgeless"])
def test_budget(name):
    g = K.case_graph(next(c for c in CASES if c["name"] == name))
    full = mirror(g)
    n = full.counts["n_entries"]
    for nt in (1, 3):
        over = mirror(g, max_entries=n - 1, n_threads=nt)
        assert over.status == "OVER_BUDGET" and over.counts["n_cliques"] == 0 and over.clique_nodes.size == 0
        ok = mirror(g, max_entries=n, n_threads=nt)
        assert ok.status == "OK" and np.array_equal(ok.clique_nodes, full.clique_nodes) and np.array_equal(ok.clique_off, full.clique_off)


def test_count_then_fetch_and_refusals():
    edges, out_off, _, _, incl = K.case_graph(next(c for c in CASES if c["name"] == "hub_65_triangles"))
    st, c = CL.hc_cliques_settings(0, 1, 0), CL.hc_cliques_counts()
    f = N.lib.hc_host_graph_cliques
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, incl.ctypes.data, C.byref(st), None, None, 0, 0, C.byref(c)) == 0
    assert (c.n_cliques, c.n_entries, c.max_clique, c.n_singletons) == (65, 195, 3, 0)
    off, nodes = np.full(66, 7, np.uint64), np.full(195, 7, np.uint32)
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, incl.ctypes.data, C.byref(st), off.ctypes.data, nodes.ctypes.data, 64, 195, C.byref(c)) == HC_ERR_ARG
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, incl.ctypes.data, C.byref(st), off.ctypes.data, nodes.ctypes.data, 65, 194, C.byref(c)) == HC_ERR_ARG
    assert (c.n_cliques, c.n_entries) == (65, 195) and (off == 7).all() and (nodes == 7).all()  # counts filled, nothing written
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, incl.ctypes.data, C.byref(st), off.ctypes.data, nodes.ctypes.data, 65, 195, C.byref(c)) == 0
    assert off[0] == 0 and off[65] == 195 and (np.diff(off.astype(np.int64)) == 3).all()
    # either array alone
    off2 = np.zeros(66, np.uint64)
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, incl.ctypes.data, C.byref(st), off2.ctypes.data, None, 65, 0, C.byref(c)) == 0
    assert np.array_equal(off2, off)
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, None, None, None, None, 0, 0, C.byref(c)) == HC_ERR_ARG
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, None, C.byref(st), None, None, 0, 0, None) == HC_ERR_ARG
    st.max_entries = 1 << 31
    assert f(edges.ctypes.data, out_off.ctypes.data, 131, None, C.byref(st), None, None, 0, 0, C.byref(c)) == HC_ERR_ARG


def test_clique_select_accepts_the_output():
    case = next(c for c in CASES if c["name"] == "interval_300")
    got = mirror(K.case_graph(case))
    sel = host_clique_select(got.clique_off, got.clique_nodes, case["n_vertices"], min_clique_size=2)
    assert sel.n_singletons == got.counts["n_singletons"]
    assert sel.clique_off.size - 1 == got.counts["n_cliques"] - got.counts["n_singletons"]
    multi = host_clique_select(got.clique_off, got.clique_nodes, case["n_vertices"], min_clique_size=2, remove_multi_occ=True)
    assert 0 < multi.clique_off.size - 1 <= sel.clique_off.size - 1
    assert np.unique(multi.clique_nodes).size == multi.clique_nodes.size
