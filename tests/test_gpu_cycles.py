"""The second sortEdges and cycleRemovalHeuristic on the device graph (hc_graph_sort_edges / hc_graph_remove_cycles /
hc_graph_fetch_cycle_pairs): every case of tests/golden/cycles.json — the reference's own output — through hc_graph_load, the two calls
and the fetches; the device against the host mirror (pinned on the CPU in tests/test_cycles_host.py) array for array — both lists,
branching_edges, the pairs, every count — on a 20 000-vertex chain, open and closed, out-lists of 63 / 64 / 65 records and a 300-record
hub on a cycle, lists of 1 024 / 1 025 / 3 000 records (the bound between the ranked and the radix-sorted columns), 2 000 acyclic components with 5 cyclic ones among them (the compact CSR and its renumbering), a fully tied list of 17
records through the sort, remove_edges = 0, and the chain hc_graph_remove_branches -> hc_graph_sort_edges -> hc_graph_remove_cycles ->
hc_graph_write_text against the mirror's chain; what the calls refuse, a graph hc_br_evidence has reordered included."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import cliques as CL
from tests import _cycles as Y
from tests import _trans

pytestmark = pytest.mark.gpu

CASES = Y.load()["cases"]


@pytest.fixture(scope="module")
def scorer():
    if hc.device_count() < 1:
        pytest.fail("no HIP device")
    with hc.EdgeScorer(hc.Settings(n_threads=8)) as sc:
        yield sc


def fetched(sc):
    f = sc.graph_fetch()
    return (f["edges"], f["out_off"], f["in_nodes"], f["in_off"]), f["seq"]


def device_sorted(sc, g, lens, n_tied=0):
    """hc_graph_load + hc_graph_sort_edges, checked against hc_host_graph_sort_edges; returns the sorted graph."""
    sc.graph_load(*g)
    counts = sc.graph_sort_edges(lens)
    got, seq = fetched(sc)
    want = Y.host_sorted(g, lens)
    assert Y.same_graph(got, want)
    assert counts == dict(n_edges=g[0].shape[0], n_tied_lists=n_tied)
    assert np.array_equal(g[0]["perc"][seq], got[0]["perc"])  # seq follows the records (hc_graph_load numbers them 0, 1, ...)
    return got


def both(sc, g, lens, remove=True, what="", n_tied=0):
    """load, sort, remove cycles on the device; the mirror on the host-sorted graph; everything equal."""
    gs = device_sorted(sc, g, lens, n_tied)
    had = sc.graph_branching_edges()
    r = sc.graph_remove_cycles(remove)
    want = Y.mirror(gs, remove, n_threads=3)
    assert {k: r.counts[k] for k in Y.COUNTS} == {k: want.counts[k] for k in Y.COUNTS}, what
    assert r.pairs.tolist() == want.pairs.tolist(), what
    got, _ = fetched(sc)
    assert Y.same_graph(got, Y.graph_of(want)), what
    br = sc.graph_branching_edges()
    assert Y.same_records(br[:had.shape[0]], had) and Y.same_records(br[had.shape[0]:], want.removed), what
    return r, want


@pytest.mark.parametrize("remove", [True, False], ids=["remove", "keep"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case(scorer, case, remove):
    recs = Y.case_records(case["edges"])
    g = Y.inserted(case["V"], recs)
    lens = np.asarray(case["len_by_read"], np.uint32)
    gs = device_sorted(scorer, g, lens)
    assert gs[0]["perc"].tolist() == case["sorted_out"] and gs[2].tolist() == case["sorted_in"]
    want = case["remove" if remove else "keep"]
    r = scorer.graph_remove_cycles(remove)
    (edges, out_off, in_nodes, in_off), _ = fetched(scorer)
    assert edges["perc"].tolist() == want["out"] and out_off.tolist() == want["out_off"]
    assert in_nodes.tolist() == want["in_nodes"] and in_off.tolist() == want["in_off"]
    assert scorer.graph_branching_edges()["perc"].tolist() == want["branching"]
    assert r.counts["backedge_count"] == want["backedge_count"] and r.status == "OK"
    txt = r.cycles_txt()
    assert (txt.decode() if txt is not None else None) == want["cycles_txt"]
    sizes = [len(s) for s in case["sets"]]
    assert r.counts["try_size"] == (sizes if sizes[0] else [0] * 20)
    assert r.counts["best_try"] == sizes.index(min(sizes)) + 1 and r.counts["tries"] == (20 if sizes[0] else 1)
    assert Y.same_records(edges, recs[edges["perc"]])


@pytest.mark.parametrize("closed", [False, True], ids=["chain", "ring"])
def test_long_chain(scorer, closed):
    V = 20000
    recs, lens = Y.chain(V, closed)
    r, _ = both(scorer, Y.inserted(V, recs), lens, True, closed)
    assert r.pairs.tolist() == ([[V - 1, 0]] if closed else [])
    assert (r.counts["tries"], r.counts["n_host_vertices"]) == ((20, V) if closed else (1, 0))


def hub_graph(seed):
    """3 000 vertices: a seeded graph, out-lists of 63 / 64 / 65 records and a hub of 300, every one of them on a cycle."""
    rng = np.random.default_rng(seed)
    V = 3000
    parts = [Y.random_records(rng, V - 100, 5000, 100)]  # (the hubs' lists are theirs alone)
    for hub, deg in ((5, 63), (6, 64), (7, 65), (8, 300)):
        t = rng.choice(np.arange(100, V), deg, replace=False)
        parts.append(Y.records(np.full(deg, hub), t, pos1=rng.integers(-3, 4, deg), len1=rng.integers(20, 40, deg), score=rng.integers(1, 5, deg) / 4.0,
                               mismatch_rate=rng.integers(0, 3, deg) / 8.0))
        parts.append(Y.records(t[:3], np.full(3, hub), pos1=[1, 2, 3]))
    return V, Y.concat(parts), rng.integers(60, 140, V).astype(np.uint32)


def test_long_lists_and_a_hub_on_a_cycle(scorer):
    V, recs, lens = hub_graph(21)
    r, want = both(scorer, Y.inserted(V, recs), lens, True, "hub")
    assert r.counts["tries"] == 20 and r.counts["backedge_count"] > 0
    hubs = {5, 6, 7, 8}
    assert hubs & set(r.pairs[:, 1].tolist()) or hubs & set(r.pairs[:, 0].tolist())


def long_list_graph(deg, seed):
    """A hub of `deg` out-records on cycles among 400 seeded vertices; keys from few values, so the target decides often."""
    rng = np.random.default_rng(seed)
    V = deg + 400
    t = 1 + rng.permutation(deg)
    parts = [Y.records(np.zeros(deg), t, pos1=rng.integers(-3, 4, deg), len1=rng.integers(20, 40, deg), score=rng.integers(1, 5, deg) / 4.0,
                       mismatch_rate=rng.integers(0, 3, deg) / 8.0),
             Y.records(t[:5], np.zeros(5), pos1=[1, 2, 3, 4, 5]), Y.random_records(rng, 400, 900, deg)]
    return V, Y.concat(parts), rng.integers(60, 140, V).astype(np.uint32)


@pytest.mark.parametrize("deg", [1024, 1025, 3000])
def test_lists_around_the_ranking_bound(scorer, deg):
    """A graph whose longest list has at most 1024 records ranks its columns inside lists; one record more and every column of the call —
    try 1's and those of tries 2 - 4 on the compact CSR — comes from the three radix sorts."""
    V, recs, lens = long_list_graph(deg, deg)
    g = Y.inserted(V, recs)
    assert int(g[1][1] - g[1][0]) == deg
    r, _ = both(scorer, g, lens, True, deg)
    assert r.counts["tries"] == 20 and 0 in set(r.pairs[:, 1].tolist())


def components_graph(seed):
    """2 000 acyclic components of 6 vertices and 5 cyclic ones of 9 scattered among them."""
    rng = np.random.default_rng(seed)
    cyclic = set(rng.choice(2005, 5, replace=False).tolist())
    parts, lo = [], 0
    for k in range(2005):
        if k in cyclic:
            ring = np.arange(9)
            parts.append(Y.records(lo + ring, lo + (ring + 1) % 9, pos1=rng.integers(-2, 3, 9)))
            parts.append(Y.random_records(rng, 9, 14, lo))
            lo += 9
        else:
            parts.append(Y.random_records(rng, 6, 8, lo, acyclic=True))
            lo += 6
    return lo, Y.concat(parts), rng.integers(60, 140, lo).astype(np.uint32)


def test_cyclic_components_among_acyclic_ones(scorer):
    V, recs, lens = components_graph(5)
    r, _ = both(scorer, Y.inserted(V, recs), lens, True, "components")
    assert (r.counts["n_flagged_components"], r.counts["n_host_vertices"], r.counts["tries"]) == (5, 45, 20)
    assert r.counts["n_host_edges"] < recs.shape[0] // 20


def test_fully_tied_list_of_17_records(scorer):
    """17 records of one (non-overlap length, target): std::sort's order of the list, which only its own code restates."""
    rng = np.random.default_rng(9)
    tied = Y.records(np.zeros(17), np.full(17, 3), pos1=rng.permutation(17), len1=30, score=rng.integers(1, 9, 17) / 8.0)
    rest = Y.records([0, 0, 3, 1, 2], [1, 2, 0, 2, 4], len1=[25, 35, 30, 30, 30])
    sixteen = Y.records(np.full(15, 1), np.full(15, 4), pos1=rng.permutation(15), len1=30)  # 16 with 1 -> 2: the incoming order stays
    recs = Y.concat([tied[:9], rest, sixteen, tied[9:]])
    lens = np.full(5, 100, np.uint32)
    both(scorer, Y.inserted(5, recs), lens, True, "tied", n_tied=1)


def test_keep_edges_leaves_the_graph_untouched(scorer):
    V, recs, lens = components_graph(6)
    g = Y.inserted(V, recs)
    gs = device_sorted(scorer, g, lens)
    r = scorer.graph_remove_cycles(False)
    got, _ = fetched(scorer)
    assert r.counts["backedge_count"] > 0 and r.counts["edges_after"] == recs.shape[0]
    assert Y.same_graph(got, gs) and scorer.graph_branching_edges().shape[0] == 0
    # the stamp holds: the same call again, now with the edit, gives the mirror's graph
    r2 = scorer.graph_remove_cycles(True)
    want = Y.mirror(gs, True)
    assert r2.pairs.tolist() == r.pairs.tolist() == want.pairs.tolist()
    assert Y.same_graph(fetched(scorer)[0], Y.graph_of(want))


def test_chain_from_branch_removal_to_graph_text(scorer):
    """hc_graph_remove_branches -> hc_graph_sort_edges -> hc_graph_remove_cycles -> hc_graph_write_text without a fetch or a load in
    between, against the mirror's chain."""
    V = 3000
    a, b = _trans.interval_edges(V, 5, seed=31)
    rng = np.random.default_rng(32)
    back = rng.choice(V - 40, 60, replace=False)
    a, b = np.concatenate([a, back + rng.integers(2, 30, 60)]), np.concatenate([b, back])  # 60 records against the tiling
    edges, out_off, in_nodes, in_off, incl = _trans.shuffled_graph(a, b, V, 33)
    incl[:] = 0
    lens = rng.integers(150, 250, V).astype(np.uint32)
    m = _trans.Mirror(edges, out_off, in_nodes, in_off, incl)
    scorer.graph_load(edges, out_off, in_nodes, in_off, incl)
    mc, dc = m.g.remove_branches(), scorer.graph_remove_branches()
    assert mc["n_removed"] == dc["n_removed"]
    with pytest.raises(hc.HcError):  # branch removal leaves target order: the stamp is not there
        scorer.graph_remove_cycles(True)
    m.g.sort_edges(lens)
    scorer.graph_sort_edges(lens)
    me, m_in_off, m_in = m.result()
    mg = (me, Y.out_offsets(me, V), m_in.astype(np.uint32), m_in_off)
    assert Y.same_graph(fetched(scorer)[0], mg)
    want = Y.mirror(mg, True, n_threads=4)
    r = scorer.graph_remove_cycles(True)
    assert r.pairs.tolist() == want.pairs.tolist() and {k: r.counts[k] for k in Y.COUNTS} == {k: want.counts[k] for k in Y.COUNTS}
    assert want.counts["backedge_count"] > 0
    m2 = _trans.Mirror(*Y.graph_of(want), incl)
    for kind in ("cliques", "digraph"):
        want_text, wc = m2.g.write_text(kind, edge_threshold=0.0)
        got_text, gc = scorer.graph_write_text(kind, edge_threshold=0.0)
        assert got_text == want_text and gc["status"] == wc["status"], kind
    # branching_edges: the branches' records, then the cycles'
    br = scorer.graph_branching_edges()
    assert Y.same_records(br, np.concatenate([m.g.branching_edges(), want.removed]))
    # and the cliques follow on the device
    dq, hq = scorer.graph_cliques(), CL.host_graph_cliques(want.edges, want.out_off, incl)
    assert dq.counts["status"] == hq.counts["status"] and dq.as_set() == hq.as_set()


def test_branch_evidence_takes_the_stamp_away():
    """hc_br_evidence leaves adj_out in target order without a cleaning call's commit: hc_graph_remove_cycles must refuse the graph until
    hc_graph_sort_edges has run again."""
    import ctypes as C

    from haploconduct_amd import _native as N
    from haploconduct_amd import cycles as CY
    from tests import _branch_evidence as T

    case = T.make_case(121, max_out=5, bubbles=1)
    g = case.graph()
    n_reads = int(max(g["edges"]["read1"].max(), g["edges"]["read2"].max())) + 1
    lens = (5000 - 7 * np.arange(n_reads)).astype(np.uint32)  # a later read is shorter: sortEdges' order is not target order
    with hc.EdgeScorer(hc.Settings(edge_threshold=0.97, min_overlap_len=10)) as sc:
        sc.sr_keep_device(True)
        sc.set_reads(case.reads())
        sc.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
        sc.sr_originals_load(*case.dict_arrays())
        sc.br_set_original_reads(*case.original_arrays())
        sc.graph_sort_edges(lens)
        first = sc.graph_remove_cycles(False)  # the stamp is there
        sorted_graph = fetched(sc)[0]
        sc.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
        assert not Y.same_records(fetched(sc)[0][0], sorted_graph[0])  # (target order is another order on this graph)
        st, c = CY.hc_cycles_settings(1, 0), CY.hc_cycles_counts()
        rc = N.lib.hc_graph_remove_cycles(sc._ctx, C.byref(st), C.byref(c))
        assert rc != 0 and CY.CYCLES_STATUS[c.status] == "NOT_SORTED" and c.edges_after == c.edges_before
        sc.graph_sort_edges(lens)
        assert Y.same_graph(fetched(sc)[0], sorted_graph)
        again = sc.graph_remove_cycles(False)
        assert again.pairs.tolist() == first.pairs.tolist() and again.counts["try_size"] == first.counts["try_size"]


def test_refusals(scorer):
    recs = Y.records([0, 1, 2], [1, 2, 0], score=[1.0, float("nan"), 1.0])
    g = Y.inserted(3, recs)
    scorer.graph_load(*g)
    with pytest.raises(hc.HcError):  # a loaded graph carries no stamp
        scorer.graph_remove_cycles(True)
    with pytest.raises(hc.HcError):  # a read beyond the lengths
        scorer.graph_sort_edges(np.full(2, 100, np.uint32))
    assert Y.same_graph(fetched(scorer)[0], g)
    scorer.graph_sort_edges(np.full(3, 100, np.uint32))
    r = scorer.graph_remove_cycles(True)
    assert (r.status, r.counts["bad_v"], r.counts["bad_pos"]) == ("NAN_KEY", 1, 0)
    assert Y.same_graph(fetched(scorer)[0], g) and scorer.graph_branching_edges().shape[0] == 0
