"""Vertex labelling on the device graph (hc_graph_label_vertices / hc_graph_fetch_orientations): every case of
tests/golden/labelling.json — the reference's own output — through hc_graph_load, the call and the two fetches; the device against the
host mirror (pinned on the CPU in tests/test_labelling_host.py) array for array on graphs with lists of 63 / 64 / 65 records and a hub,
a 20 000-vertex chain of alternating classes, the same chain closed into an odd cycle (one inconsistent component through the host's
walk) and 500 small components of which 5 are inconsistent; the cleaning calls on the result; the two statuses."""
import numpy as np
import pytest

import haploconduct_amd as hc
from tests import _labelling as L
from tests import _trans

pytestmark = pytest.mark.gpu

CASES = L.load()["cases"]


@pytest.fixture(scope="module")
def scorer():
    if hc.device_count() < 1:
        pytest.fail("no HIP device")
    with hc.EdgeScorer(hc.Settings(n_threads=8)) as sc:
        yield sc


def device(sc, g, flags=2, n_reads=0, inclusions=None):
    sc.graph_load(*g, inclusions)
    counts = sc.graph_label_vertices(bool(flags & 2), bool(flags & 1), n_reads)
    f = sc.graph_fetch()
    fwd = sc.graph_orientations() if counts["status"] != 2 else None
    return (f["edges"], f["out_off"], f["in_nodes"], f["in_off"]), fwd, counts, f["seq"]


def both(sc, g, what):
    got, fwd, counts, seq = device(sc, g)
    want, want_fwd, want_counts = L.mirror(g)
    assert {k: counts[k] for k in L.COUNTS} == {k: want_counts[k] for k in L.COUNTS}, what
    assert L.same_graph(got, want), what
    assert np.array_equal(fwd, want_fwd), what
    assert np.array_equal(g[0]["perc"][seq], got[0]["perc"]), what  # seq follows the records
    return counts


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case(scorer, case):
    g = L.graph(case["V"], case["edges"])
    (edges, out_off, in_nodes, in_off), fwd, counts, seq = device(scorer, g, case["flags"], case["n_reads"])
    assert L.golden_rows(edges) == case["out"]
    assert out_off.tolist() == case["out_off"] and in_off.tolist() == case["in_off"] and in_nodes.tolist() == case["in_nodes"]
    assert fwd.tolist() == case["orientations"]
    assert counts["edges_after"] == case["edge_count"] and counts["conflict_count"] == case["conflict_count"]
    assert counts["tries"] == case["tries"] and counts["n_moved"] == len(case["moved"])
    assert (counts["status"], counts["bad_v"], counts["bad_pos"]) == (case["status"], case["bad_v"], case["bad_pos"])
    assert np.array_equal(g[0]["perc"][seq], edges["perc"])
    for f in ("score", "mismatch_rate", "len0", "len1", "len2"):
        assert np.array_equal(edges[f], g[0][f][edges["perc"]])


def hub_graph(seed):
    """3 000 vertices: a seeded graph with a hidden labelling, out-lists of 63 / 64 / 65 records and one hub of 300."""
    rng = np.random.default_rng(seed)
    V = 3000
    edges = L.random_edges(rng, V, 7000, 0, 1)
    have = {(e["v1"], e["v2"]) for e in edges} | {(e["v2"], e["v1"]) for e in edges}
    for hub, deg in ((5, 63), (6, 64), (7, 65), (8, 300)):
        for t in rng.choice(np.arange(100, V), deg, replace=False).tolist():
            if (hub, t) not in have:
                have.update(((hub, t), (t, hub)))
                edges.append(dict(v1=hub, v2=t, ori1=1, ori2=int(rng.integers(0, 2)), pos1=3, pos2=0, pos3=int(rng.choice((-2, 0, 3))), pos4=0, ord="-"))
    return V, edges


def chain(V, closed):
    """i -> i + 1 with alternating classes; closed: the record V - 1 -> 0 of the class that makes the cycle odd."""
    edges = [dict(v1=i, v2=i + 1, ori1=1, ori2=1 - (i & 1), pos1=4, pos2=0, pos3=(-1, 0, 2)[i % 3], pos4=0, ord="-") for i in range(V - 1)]
    if closed:
        crossed = sum(e["ori1"] != e["ori2"] for e in edges)
        edges.append(dict(v1=V - 1, v2=0, ori1=1, ori2=1 if crossed % 2 else 0, pos1=4, pos2=0, pos3=2, pos4=0, ord="-"))
    return edges


def test_lists_of_63_64_65_and_a_hub(scorer):
    V, edges = hub_graph(11)
    g = L.graph(V, edges)
    deg = np.diff(g[1].astype(np.int64))
    assert deg.max() >= 300 and all((deg >= d).sum() >= 1 for d in (63, 64, 65))
    # the hubs' records take either class: the giant component is inconsistent, and the host's walk shuffles lists of these lengths
    counts = both(scorer, g, "hub")
    assert counts["n_moved"] > 0 and counts["tries"] == 100


def test_chain_of_alternating_classes(scorer):
    counts = both(scorer, L.graph(20000, chain(20000, False)), "chain")
    assert (counts["tries"], counts["n_components"], counts["n_inconsistent"], counts["n_host_vertices"]) == (1, 1, 0, 0)


def test_odd_cycle_goes_through_the_hosts_walk(scorer):
    counts = both(scorer, L.graph(20000, chain(20000, True)), "odd cycle")
    assert (counts["tries"], counts["n_inconsistent"], counts["n_host_vertices"], counts["n_host_edges"]) == (100, 1, 20000, 20000)
    assert counts["conflict_count"] >= 1


def test_small_components_five_inconsistent(scorer):
    rng = np.random.default_rng(3)
    edges, first, odd_size = [], 0, 0
    for k in range(500):
        n = int(rng.integers(3, 9))
        n_odd = 1 if k % 100 == 7 else 0
        part = L.random_edges(rng, n, 2 * n, n_odd, 1)
        for e in part:
            e["v1"] += first
            e["v2"] += first
        edges += part
        first += n
        odd_size += n if n_odd else 0
    counts = both(scorer, L.graph(first, edges), "small components")
    assert counts["n_components"] == 500 and counts["n_inconsistent"] == 5
    assert counts["n_host_vertices"] == odd_size


def test_cleaning_calls_on_the_result(scorer):
    rng = np.random.default_rng(9)
    V = 400
    g = L.graph(V, L.random_edges(rng, V, 1400, 3, 2))
    incl = (rng.random(V) < 0.05).astype(np.uint8)
    device(scorer, g, inclusions=incl)
    m = _trans.Mirror(*g, incl)
    m.g.label_vertices()

    def same(what):
        f = scorer.graph_fetch()
        edges, in_off, in_nodes = m.result()
        assert all(np.array_equal(f["edges"][k], edges[k]) for k in L.ALL_FIELDS), what
        assert np.array_equal(f["in_off"], in_off) and np.array_equal(f["in_nodes"], in_nodes.astype(np.uint32)), what

    same("labelled")
    scorer.graph_remove_inclusions()
    m.remove_inclusions()
    same("removeInclusions")
    scorer.graph_remove_transitive(1, False)
    m.remove_transitive(1, False)
    same("removeTransitiveEdges")


def test_no_graph_is_a_state_error():
    with hc.EdgeScorer(hc.Settings()) as sc:
        for call in (sc.graph_label_vertices, sc.graph_orientations):
            with pytest.raises(hc.HcError) as err:
                call()
            assert err.value.status == -5  # HC_ERR_STATE


def test_statuses(scorer):
    e0 = CASES[0]["edges"][0]
    # a record that repeats the (target, class) of an earlier one of its list: refused, nothing changed, no orientations kept
    edges = [dict(e0, v1=0, v2=1), dict(e0, v1=2, v2=3), dict(e0, v1=2, v2=4), dict(e0, v1=2, v2=3, pos1=1), dict(e0, v1=2, v2=3)]
    g = L.graph(5, edges)
    got, fwd, counts, _ = device(scorer, g)
    assert (counts["status"], counts["bad_v"], counts["bad_pos"]) == (2, 2, 2) and L.same_graph(got, g)
    with pytest.raises(hc.HcError):
        scorer.graph_orientations()
    # checkDuplicateEdges after a labelling that moved records: the graph is re-labelled all the same
    # (2 -> 1 turns round and lands behind 1 -> 2)
    edges = [dict(e0, v1=0, v2=1), dict(e0, v1=2, v2=1, ori1=0, ori2=0, pos3=-1), dict(e0, v1=1, v2=3), dict(e0, v1=1, v2=2)]
    g = L.graph(4, edges)
    got, fwd, counts, _ = device(scorer, g)
    want, want_fwd, want_counts = L.mirror(g)
    assert (counts["status"], counts["bad_v"], counts["bad_pos"], counts["n_moved"]) == (1, 1, 2, 1)
    assert {k: counts[k] for k in L.COUNTS} == {k: want_counts[k] for k in L.COUNTS}
    assert L.same_graph(got, want) and np.array_equal(fwd, want_fwd)
