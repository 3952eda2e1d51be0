"""Maximal cliques on the device graph (hc_graph_cliques / hc_graph_cliques_fetch) against the host mirror, array for array — the
mirror itself is pinned on the CPU against quick-cliques' own output, an exhaustive check and the restated rule
(tests/test_cliques_host.py).  Every golden graph; root universes on both sides of the 64-bit word boundaries, as complete graphs and
with exponentially many cliques; roots above root_cap on the host route; empty and edgeless graphs; a 20 000-vertex interval graph;
the budget; the result fed to hc_sr_clique_merge; a second call after the graph was cleaned.  In every test but the root_cap ones,
n_host_roots == 0 is a condition."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import cliques as CL
from haploconduct_amd.clique_next import host_clique_select
from tests import _cliques as K

pytestmark = pytest.mark.gpu

CASES = K.load_cases()
SAME = ("status", "bad_v", "bad_pos", "n_pairs", "n_cliques", "n_entries", "n_singletons", "max_clique")


@pytest.fixture(scope="module")
def scorer():
    if hc.device_count() < 1:
        pytest.fail("no HIP device")
    with hc.EdgeScorer(hc.Settings()) as sc:
        yield sc


def both(sc, g, what, host_roots=0, **kw):
    """Loads the graph; (device result, mirror result), equal array for array and count for count."""
    sc.graph_load(*g)
    got = sc.graph_cliques(**kw)
    want = CL.host_graph_cliques(g[0], g[1], g[4], max_entries=kw.get("max_entries", 0))
    assert {k: got.counts[k] for k in SAME} == {k: want.counts[k] for k in SAME}, what
    assert got.counts["n_host_roots"] == host_roots, (what, got.counts)
    assert np.array_equal(got.clique_off, want.clique_off), what
    assert np.array_equal(got.clique_nodes, want.clique_nodes), what
    return got, want


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_device_equals_mirror_on_every_golden_graph(scorer, name):
    case = next(c for c in CASES if c["name"] == name)
    got, _ = both(scorer, K.case_graph(case), name)
    assert got.status == "OK" and got.as_set() == set(K.qc_cliques(case["qc_stdout"])[0])
    assert got.counts["ms_device"] > 0


def padded_matching(U):
    """Root 0 with a universe of U neighbours: a core of 20 (K20 minus a perfect matching: 2^10 cliques), ten of them the smallest and ten
    the largest local indices, and U - 20 pendant neighbours between them.  Every core vertex has U leaves of its own, so that it ranks
    above the root."""
    core = list(range(1, 11)) + list(range(U - 9, U + 1))
    pairs = [(0, u) for u in range(1, U + 1)]
    pairs += [(core[a], core[b]) for a in range(20) for b in range(a + 1, 20) if a ^ 1 != b]
    nxt = U + 1
    for u in core:
        pairs += [(u, nxt + k) for k in range(U)]
        nxt += U
    return nxt, pairs


@pytest.mark.parametrize("U", [63, 64, 65, 127, 128, 129])
def test_universes_at_the_word_boundaries(scorer, U):
    got, _ = both(scorer, K.graph(U + 2, K.complete(U + 1)), f"K{U + 1}")  # the root of K_(U+1) has U neighbours
    assert got.counts["n_cliques"] == 2 and got.counts["max_clique"] == U + 1
    V, pairs = padded_matching(U)
    got, _ = both(scorer, K.graph(V, pairs), f"matching form, U = {U}")
    rows = [got.row(k) for k in range(got.clique_off.size - 1)]
    assert sum(r.size == 11 and r[0] == 0 for r in rows) == 1024 and got.counts["max_clique"] == 11


def expected_host_roots(V, pairs, cap):
    nb = [set() for _ in range(V)]
    for a, b in pairs:
        nb[a].add(b), nb[b].add(a)
    key = [(len(nb[v]), v) for v in range(V)]
    return sum(len(nb[v]) > cap and any(key[u] > key[v] for u in nb[v]) for v in range(V))


@pytest.mark.parametrize("name,cap,n_host", [("k65", 64, 0), ("k65", 63, 64), ("k129", 64, 128), ("hub_65_triangles", 64, 0), ("hub_65_triangles", 1, None), ("k129", 1 << 30, 0),
                                             ("interval_300", 16, None), ("gnp_40_0", 20, None), ("moon_moser_5x3", 2, 12)])
def test_roots_above_root_cap_go_to_the_host(scorer, name, cap, n_host):
    """A root goes to the host iff its degree is above root_cap and a neighbour ranks above it (the hub of the triangles has the largest
    degree: nothing ranks above it, it yields nothing and is nobody's work).  The output does not depend on the route.  A root_cap above
    HC_CLIQUES_MAX_ROOT_CAP is taken as that."""
    case = next(c for c in CASES if c["name"] == name)
    want_host = expected_host_roots(case["n_vertices"], K.pair_set(case["n_vertices"], case["edges"]), cap)
    assert n_host is None or n_host == want_host
    assert n_host == 0 or want_host > 0
    g = K.case_graph(case)
    got, _ = both(scorer, g, (name, cap), host_roots=want_host, root_cap=cap, n_threads=3)
    assert want_host == 0 or got.counts["ms_host"] > 0
    again, _ = both(scorer, g, (name, "default cap"))
    assert np.array_equal(got.clique_nodes, again.clique_nodes) and np.array_equal(got.clique_off, again.clique_off)


def test_empty_and_edgeless_graphs(scorer):
    got, _ = both(scorer, K.graph(0, []), "no vertices")
    assert got.counts["n_cliques"] == 0 and np.array_equal(got.clique_off, [0])
    got, _ = both(scorer, K.graph(5, [], incl=[1, 1, 1, 1, 1]), "inclusion vertices only")
    assert got.as_set() == {(v,) for v in range(5)}
    V = 100000
    got, _ = both(scorer, K.graph(V, []), "isolated vertices")
    assert got.counts["n_cliques"] == got.counts["n_singletons"] == V and np.array_equal(got.clique_nodes, np.arange(V))


def test_interval_graph_of_20000_vertices(scorer):
    V = 20000
    got, _ = both(scorer, K.graph(V, K.interval_pairs(V, 60, seed=4)), "interval graph")
    assert 0 < got.counts["n_cliques"] <= V and got.counts["max_clique"] >= 5


def test_statuses_and_budget(scorer):
    got, _ = both(scorer, K.graph(900, [(0, 1), (700, 3), (700, 700), (4, 4), (2, 5)]), "self-loop")
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("SELF_LOOP", 4, 0)
    got, _ = both(scorer, K.graph(900, [(0, 1), (700, 3), (700, 700), (800, 5)], incl=[0] * 40 + [1] + [0] * 859), "self-loop 700")
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("SELF_LOOP", 700, 1)
    got, _ = both(scorer, K.graph(900, [(0, 1), (40, 3), (700, 700)], incl=[0] * 40 + [1] + [0] * 859), "inclusion with edges")
    assert (got.status, got.counts["bad_v"], got.counts["bad_pos"]) == ("INCLUSION_HAS_EDGES", 40, 0)
    assert hc._native.lib.hc_graph_cliques_fetch(scorer._ctx, None, None) == -5  # nothing kept
    g = K.case_graph(next(c for c in CASES if c["name"] == "moon_moser_5x3"))
    over, _ = both(scorer, g, "over budget", max_entries=1216)
    assert over.status == "OVER_BUDGET" and over.counts["n_cliques"] == 0
    assert hc._native.lib.hc_graph_cliques_fetch(scorer._ctx, None, None) == -5
    ok, _ = both(scorer, g, "at the budget", max_entries=1217)
    assert ok.status == "OK" and ok.counts["n_entries"] == 1217
    g2 = K.case_graph(next(c for c in CASES if c["name"] == "interval_2000"))  # enough roots for the early stop
    over, _ = both(scorer, g2, "over budget early", max_entries=100)
    assert over.status == "OVER_BUDGET"


def test_clique_merge_takes_the_device_csr():
    """hc_sr_clique_merge fed hc_graph_cliques_fetch's arrays through the gate, on a store whose overlap graph has cliques of three to
    five reads: every clique's status is OK and the layouts are those of the host's clique merge (hc_host_sr_clique_merge_layouts) fed
    the MIRROR's CSR — an independent route: host enumeration, host layouts."""
    from haploconduct_amd import consensus as SR
    from haploconduct_amd import host
    from tests import _clique_merge as CM
    from tests import _edge_merge as EM

    reads, V, rows, vertex_read, vertex_fwd = K.overlap_graph()
    csr = EM.csr(V, rows)
    mir = CL.host_graph_cliques(csr[0], csr[1])
    want_sel = host_clique_select(mir.clique_off, mir.clique_nodes, V, min_clique_size=2)
    sizes = np.diff(want_sel.clique_off.astype(np.int64))
    assert sizes.size > 40 and sizes.min() >= 3 and sizes.max() >= 5  # triangles and more reach the merge
    st = SR.make_settings(min_clique_size=2)
    args = (csr[0], csr[1], reads, want_sel.clique_off, want_sel.clique_nodes, vertex_read, vertex_fwd, st)
    first = SR.host_clique_merge_layouts(*args)
    cons = host.sr_consensus(reads, *first.used_layouts(), min_clique_size=2, n_threads=4)
    want = SR.host_clique_merge_layouts(*args, ret=cons.ret)
    assert (want.clique_status == SR.SR_EDGE_OK).all()
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        sc.graph_load(*csr)
        dev = sc.graph_cliques()
        assert dev.status == "OK" and dev.counts["n_host_roots"] == 0
        sel = host_clique_select(dev.clique_off, dev.clique_nodes, V, min_clique_size=2)
        got = sc.sr_clique_merge(sel.clique_off, sel.clique_nodes, vertex_read, vertex_fwd, min_clique_size=2)
        assert got.clique_status.size == sizes.size and (got.clique_status == SR.SR_EDGE_OK).all(), got.clique_status
        assert np.array_equal(got.result.ret, cons.ret)
        CM.assert_equal_layouts(got, want, "device cliques and merge against the host's")
        # the cliques outlive the merge: the graph is as it was
        off = np.zeros(dev.clique_off.size, np.uint64)
        hc._native.check(hc._native.lib.hc_graph_cliques_fetch(sc._ctx, off.ctypes.data, None), "hc_graph_cliques_fetch")
        assert np.array_equal(off, dev.clique_off)


def test_second_call_after_the_graph_was_cleaned(scorer):
    """hc_graph_remove_transitive drops the kept CSR; the next call returns the new graph's cliques."""
    from tests import _trans

    V = 400
    v1, v2 = _trans.interval_edges(V, 6, seed=8)
    g = (*_trans.csr_from_inserts(_trans.make_records(v1, v2, 2), V), np.zeros(V, np.uint8))
    first, _ = both(scorer, g, "before cleaning")
    counts = scorer.graph_remove_transitive(1)
    assert counts["transitive_count"] > 0
    assert hc._native.lib.hc_graph_cliques_fetch(scorer._ctx, None, None) == -5  # the old graph's cliques are gone
    cleaned = scorer.graph_fetch()
    got = scorer.graph_cliques()
    want = CL.host_graph_cliques(cleaned["edges"], cleaned["out_off"], cleaned["inclusions"])
    assert got.counts["n_host_roots"] == 0 and got.counts["n_pairs"] < first.counts["n_pairs"]
    assert np.array_equal(got.clique_off, want.clique_off) and np.array_equal(got.clique_nodes, want.clique_nodes)
    assert got.as_set() != first.as_set()
