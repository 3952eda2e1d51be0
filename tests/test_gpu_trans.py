"""removeInclusions + removeTransitiveEdges on the device (hc_graph_load / hc_graph_remove_inclusions /
hc_graph_remove_transitive / hc_graph_fetch_inclusion_edges) against the reference's results
(tests/golden/trans_edges.json) and against the host mirror on large seeded graphs: hubs beyond any LDS tile,
repeated targets in long lists (std::sort's order), add_duplicates graphs, both removal branches, remove_trans 1/2/3
with and without branch reduction, inclusions."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import host
from haploconduct_amd.records import FLAG_IGNORE_INCLUSIONS, FLAG_RESOLVE_ORIENTATIONS
from tests import _trans
from tests.test_gpu_graph import _admitted, _host_edges

pytestmark = pytest.mark.gpu

CASES = _trans.load_cases()


@pytest.fixture(scope="module")
def scorer():
    if hc.device_count() < 1:
        pytest.fail("no HIP device")
    with hc.EdgeScorer(hc.Settings()) as sc:
        yield sc


def device_clean(sc, edges, out_off, in_nodes, in_off, incl, rt, br, do_incl):
    sc.graph_load(edges, out_off, in_nodes, in_off, incl if do_incl else None)
    groups = None
    if do_incl:
        ic = sc.graph_remove_inclusions()
        groups = sc.graph_inclusion_edges()
        assert ic["edges_before"] - ic["del_count"] == ic["edges_after"]
    counts = sc.graph_remove_transitive(rt, br)
    return sc.graph_fetch(), counts, groups


def mirror_clean(edges, out_off, in_nodes, in_off, incl, rt, br, do_incl):
    m = _trans.Mirror(edges, out_off, in_nodes, in_off, incl if do_incl else None)
    groups = m.remove_inclusions() if do_incl else None
    counts = m.remove_transitive(rt, br)
    out, ioff, inodes = m.result()
    return out, ioff, inodes, counts, groups


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_device_equals_reference(scorer, name):
    case = next(c for c in CASES if c["name"] == name)
    V = case["V"]
    recs = _trans.golden_records(case["edges_in"])
    edges, out_off, in_nodes, in_off = _trans.csr_from_inserts(recs, V)
    for var in case["variants"]:
        got, counts, groups = device_clean(scorer, edges, out_off, in_nodes, in_off, np.array(case["incl"], np.uint8), var["remove_trans"],
                                           var["branch_reduction"], var["inclusions"])
        where = f"{name} {var['remove_trans']}/{var['branch_reduction']}/{var['inclusions']}"
        assert counts["edges_after"] == var["edge_count"], where
        assert counts["transitive_count"] == var["transitive_count"], where
        assert _trans.same_records(got["edges"], recs[var["out"]]), where
        assert got["out_off"].tolist() == var["out_off"], where
        assert got["in_off"].tolist() == var["in_off"] and got["in_nodes"].tolist() == var["in_nodes"], where
        assert edges["pos4"][got["seq"]].tolist() == var["out"], where  # seq: the place of each record in the loaded graph
        if var["inclusions"]:
            gv, goff, gedges = groups
            assert gv.tolist() == var["group_vertex"] and goff.tolist() == var["group_off"], where
            assert _trans.same_records(gedges, recs[var["group_edges"]]), where


def _graphs():
    V = 30000
    a, b = _trans.interval_edges(V, 6, seed=1)
    yield "interval", V, a, b, 0.0
    yield "interval_incl", V, a, b, 0.03
    rng = np.random.default_rng(2)
    Vs = 60000
    s1, s2 = rng.integers(0, Vs, 150000), rng.integers(0, Vs, 150000)
    ok = s1 != s2
    yield "sparse", Vs, s1[ok], s2[ok], 0.01
    Vh = 12000
    a, b = _trans.interval_edges(Vh, 4, seed=3)
    hub_out = np.full(6000, 17)
    hub_out_t = rng.choice(np.arange(18, Vh), 6000, replace=False)
    hub_in_s = rng.choice(np.arange(0, Vh - 40), 5000, replace=False)
    hub_in = np.full(5000, Vh - 20)
    yield "hubs", Vh, np.concatenate([a, hub_out, hub_in_s]), np.concatenate([b, hub_out_t, hub_in]), 0.01
    # repeated targets: a third of the edges again (the other orientation class), long lists among them
    Vr = 8000
    a, b = _trans.interval_edges(Vr, 10, seed=4)
    rep = rng.random(len(a)) < 0.33
    extra_s, extra_t = np.full(4500, 5), rng.choice(np.arange(6, Vr), 4500, replace=False)
    extra_rep = rng.random(4500) < 0.5
    yield "repeated", Vr, np.concatenate([a, a[rep], extra_s, extra_s[extra_rep]]), np.concatenate([b, b[rep], extra_t, extra_t[extra_rep]]), 0.02
    # add_duplicates: every edge mirrored between the reverse-complement copies [n, 2n)
    n = 10000
    a, b = _trans.interval_edges(n, 8, seed=5)
    yield "add_duplicates", 2 * n, np.concatenate([a, b + n]), np.concatenate([b, a + n]), 0.0
    # a caller's multigraph: pairs repeated hundreds of times, in lists far longer than 16 (std::sort's order over long runs)
    Vm = 3000
    a, b = _trans.interval_edges(Vm, 8, seed=6)
    yield "many_copies", Vm, np.concatenate([a, np.full(300, 0), np.full(200, 3), np.full(40, 7)]), \
        np.concatenate([b, np.full(300, 5), np.full(200, 9), np.full(40, 2999)]), 0.01


GRAPHS = list(_graphs())
VARIANTS = [(1, 0), (1, 1), (2, 0), (3, 0)]


@pytest.mark.parametrize("gi", range(len(GRAPHS)), ids=[g[0] for g in GRAPHS])
def test_device_equals_mirror(scorer, gi):
    name, V, v1, v2, frac = GRAPHS[gi]
    edges, out_off, in_nodes, in_off, incl = _trans.shuffled_graph(v1, v2, V, seed=gi + 10, inclusion_frac=frac)
    do_incl = frac > 0
    seen = set()
    for rt, br in VARIANTS:
        got, counts, groups = device_clean(scorer, edges, out_off, in_nodes, in_off, incl, rt, br, do_incl)
        out, ioff, inodes, mc, mgroups = mirror_clean(edges, out_off, in_nodes, in_off, incl, rt, br, do_incl)
        where = f"{name} rt={rt} br={br}"
        for k in ("edges_after", "transitive_count", "del_count", "rebuilt", "n_tied_lists"):
            assert counts[k] == mc[k], (where, k, counts, mc)
        assert _trans.same_records(got["edges"], out), where
        assert np.array_equal(got["in_off"], ioff) and np.array_equal(got["in_nodes"], inodes.astype(np.uint32)), where
        assert np.array_equal(got["edges"]["pos4"], edges["pos4"][got["seq"]]), where  # seq: the loaded record each one is
        if do_incl:
            gv, goff, gedges = groups
            moff, medges = mgroups
            assert np.array_equal(goff, moff) and _trans.same_records(gedges, medges), where
        seen.add(mc["rebuilt"])
        if name == "repeated":
            assert mc["n_tied_lists"] > 0
        if name == "hubs":
            assert np.diff(out_off).max() >= 4096 and np.diff(in_off).max() >= 4096
    if name in ("interval", "sparse"):
        assert seen == ({1, 0} if name == "interval" else {0}), seen


def _mirror_of(edges, out_off, in_nodes, in_off, incl, rt, br):
    return mirror_clean(edges, out_off, in_nodes, in_off, incl, rt, br, True)


def _same_as_mirror(got, counts, groups, want):
    out, ioff, inodes, mc, mgroups = want
    for k in ("edges_after", "transitive_count", "del_count", "rebuilt"):
        assert counts[k] == mc[k], (k, counts, mc)
    assert _trans.same_records(got["edges"], out)
    assert np.array_equal(got["in_off"], ioff) and np.array_equal(got["in_nodes"], inodes.astype(np.uint32))
    gv, goff, gedges = groups
    assert np.array_equal(goff, mgroups[0]) and _trans.same_records(gedges, mgroups[1])


def _out_off(edges, V):
    return np.concatenate([[0], np.cumsum(np.bincount(edges["v1"].astype(np.int64), minlength=V))]).astype(np.uint64)


def test_resolved_graph_route():
    """The graph hc_graph_resolve leaves: in insertion order it is cleaned as it stands (equal to the host mirror on the
    fetched graph); in sortEdges order with tied lists (whose std::sort order only the host knows) both clean calls refuse
    with HC_ERR_STATE and leave the graph alone, and the host's lists loaded with hc_graph_load clean like the mirror."""
    V, m = 300, 40000
    reads, adm = _admitted(1, V, m, 0.0)
    st = hc.Settings(edge_threshold=0.97, flags=FLAG_RESOLVE_ORIENTATIONS | FLAG_IGNORE_INCLUSIONS)
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        got = sc.graph_resolve(adm, V)
        assert got["counts"]["first_bad"] == -1 and got["inclusions"].sum() > 0
        want = _mirror_of(got["edges"], got["out_off"], got["in_nodes"], got["in_off"], got["inclusions"], 1, True)
        ic = sc.graph_remove_inclusions()
        groups = sc.graph_inclusion_edges()
        counts = sc.graph_remove_transitive(1, True)
        assert ic["del_count"] > 0 and counts["transitive_count"] > 0
        _same_as_mirror(sc.graph_fetch(), counts, groups, want)

        sgot = sc.graph_resolve(adm, V, sorted_order=True)
        assert sgot["counts"]["n_tied_lists"] > 0
        for call in (sc.graph_remove_inclusions, lambda: sc.graph_remove_transitive(1, True)):
            with pytest.raises(hc.HcError) as err:
                call()
            assert err.value.status == -5  # HC_ERR_STATE
        still = sc.graph_fetch()
        assert still["edges"].tobytes() == sgot["edges"].tobytes() and np.array_equal(still["in_nodes"], sgot["in_nodes"])
        # the host's sortEdges lists instead
        edges, len_by_read = _host_edges(reads, adm)
        g = host.HostGraph(V, st)
        for k in range(m):
            assert g.insert(edges[k]) == 0
        g.sort_edges(len_by_read)
        hedges, hinc, _ = g.get()
        hoff, hnodes = g.in_lists(hedges.size)
        out_off = _out_off(hedges, V)
        for rt, br in ((1, True), (2, False)):
            want = _mirror_of(hedges, out_off, hnodes.astype(np.uint32), hoff, hinc, rt, br)
            sc.graph_load(hedges, out_off, hnodes.astype(np.uint32), hoff, hinc)
            sc.graph_remove_inclusions()
            groups = sc.graph_inclusion_edges()
            counts = sc.graph_remove_transitive(rt, br)
            assert counts["n_tied_lists"] > 0
            _same_as_mirror(sc.graph_fetch(), counts, groups, want)


def test_load_refuses_an_inconsistent_graph(scorer):
    """hc_graph_load's device checks: an in-list that does not hold the out-lists' pairs, a record in the wrong list."""
    v1, v2 = _trans.interval_edges(500, 6, seed=7)
    edges, out_off, in_nodes, in_off, _ = _trans.shuffled_graph(v1, v2, 500, seed=7)
    scorer.graph_load(edges, out_off, in_nodes, in_off)
    bad_in = in_nodes.copy()
    bad_in[10] = (bad_in[10] + 1) % 500
    with pytest.raises(hc.HcError) as err:
        scorer.graph_load(edges, out_off, bad_in, in_off)
    assert err.value.status == -1  # HC_ERR_ARG
    with pytest.raises(hc.HcError):
        scorer.graph_remove_transitive(1)  # nothing left on the device
    bad_e = edges.copy()
    bad_e["v1"][0] = (int(bad_e["v1"][0]) + 1) % 500
    with pytest.raises(hc.HcError):
        scorer.graph_load(bad_e, out_off, in_nodes, in_off)
