"""removeTips + removeBranches on the device (hc_graph_remove_tips / hc_graph_remove_branches / hc_graph_fetch_branching_edges /
hc_graph_fetch_tip_reads) against the reference's results (tests/golden/tips_branches.json), against the host mirror on
seeded graphs at the sizes where the kernels change path (lists of 63 / 64 / 65 entries, hubs beyond one wave, repeated
pairs in long lists, add_duplicates), the component labelling on long chains and a cycle, the branching edges through
FNO=1, and the refusals."""
import math
import os

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import fno as F
from haploconduct_amd.host import READ_GEOM_DTYPE
from haploconduct_amd.records import FLAG_IGNORE_INCLUSIONS, FLAG_RESOLVE_ORIENTATIONS
from tests import _tips, _trans
from tests.test_gpu_graph import _admitted

pytestmark = pytest.mark.gpu

CASES = _tips.load_cases()


@pytest.fixture(scope="module")
def scorer():
    if hc.device_count() < 1:
        pytest.fail("no HIP device")
    with hc.EdgeScorer(hc.Settings()) as sc:
        yield sc


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_device_equals_reference(scorer, name):
    case = next(c for c in CASES if c["name"] == name)
    V = case["V"]
    recs = _tips.golden_records(case["edges_in"])
    geom = _tips.read_geom(case["reads"])
    edges, out_off, in_nodes, in_off = _trans.csr_from_inserts(recs, V)
    for vname, steps in _tips.VARIANTS.items():
        var = case["variants"][vname]
        got = _tips.device_run(scorer, edges, out_off, in_nodes, in_off, steps, case["max_tip_len"], geom)
        where = f"{name} {vname}"
        assert _trans.same_records(got["edges"], recs[var["out"]]), where
        assert got["out_off"].tolist() == var["out_off"], where
        assert got["in_off"].tolist() == var["in_off"] and got["in_nodes"].tolist() == var["in_nodes"], where
        assert edges["pos4"][got["seq"]].tolist() == var["out"], where  # seq: the place of each record in the loaded graph
        assert _trans.same_records(got["branching"], recs[var["branching"]]), where
        assert got["tips"].tolist() == var["tip_reads"], where
        _tips.check_counts(got["counts"], var, where)


def _graphs():
    rng = np.random.default_rng(11)
    V = 5000
    a, b = _trans.interval_edges(V, 4, seed=1)
    yield "interval", V, a, b, None
    # hubs beyond one wave and beyond any LDS tile: a 4 500-entry out-list and a 4 500-entry in-list
    Vh = 6000
    a, b = _trans.interval_edges(Vh, 3, seed=2)
    hub_t = rng.choice(np.arange(18, Vh), 4500, replace=False)
    yield "hub_out", Vh, np.concatenate([a, np.full(4500, 17)]), np.concatenate([b, hub_t]), None
    hub_s = rng.choice(np.arange(0, Vh - 40), 4500, replace=False)
    yield "hub_in", Vh, np.concatenate([a, hub_s]), np.concatenate([b, np.full(4500, Vh - 20)]), None
    # repeated pairs, lists longer than 16 among them (std::sort's order)
    Vr = 3000
    a, b = _trans.interval_edges(Vr, 10, seed=3)
    rep = rng.random(len(a)) < 0.33
    es, et = np.full(300, 5), rng.choice(np.arange(6, Vr), 300, replace=False)
    er = rng.random(300) < 0.5
    yield "repeated", Vr, np.concatenate([a, a[rep], es, es[er]]), np.concatenate([b, b[rep], et, et[er]]), None
    # add_duplicates: every edge once more between the reverse-complement copies [n, 2n); two vertices per read
    n = 2500
    a, b = _trans.interval_edges(n, 5, seed=4)
    yield "add_duplicates", 2 * n, np.concatenate([a, b + n]), np.concatenate([b, a + n]), n
    # lists of exactly 63 / 64 / 65 entries on both sides (the lane / wave boundary of the per-list sums): their vertices lie
    # beyond the backbone's, so nothing else enters or leaves them
    Vl = 1200
    a, b = _trans.interval_edges(1000, 2, seed=5)
    s, t = [a], [b]
    for k, d in enumerate((63, 64, 65)):
        s += [np.full(d, 1100 + k), 500 + rng.choice(400, d, replace=False)]
        t += [100 + rng.choice(400, d, replace=False), np.full(d, 1150 + k)]
    yield "lists_63_64_65", Vl, np.concatenate(s), np.concatenate(t), None


GRAPHS = list(_graphs())
STEPS = [("tips",), ("branches",), ("tips", "branches"), ("inclusions", "transitive", "tips", "branches")]


def _seeded(gi):
    name, V, v1, v2, n_reads = GRAPHS[gi]
    edges, out_off, in_nodes, in_off, incl = _trans.shuffled_graph(v1, v2, V, seed=gi + 30, inclusion_frac=0.02)
    if n_reads:
        edges["read1"], edges["read2"] = edges["v1"] % n_reads, edges["v2"] % n_reads
    edges, geom = _tips.tip_geometry(edges, V, n_reads or V, seed=gi + 40)
    return name, edges, out_off, in_nodes, in_off, incl, geom


@pytest.mark.parametrize("gi", range(len(GRAPHS)), ids=[g[0] for g in GRAPHS])
def test_device_equals_mirror(scorer, gi):
    name, edges, out_off, in_nodes, in_off, incl, geom = _seeded(gi)
    deg_out, deg_in = np.diff(out_off.astype(np.int64)), np.diff(in_off.astype(np.int64))
    if name == "hub_out":
        assert deg_out.max() >= 4500
    if name == "hub_in":
        assert deg_in.max() >= 4500
    if name == "lists_63_64_65":
        assert {63, 64, 65} <= set(deg_out.tolist()) and {63, 64, 65} <= set(deg_in.tolist())
    for steps in STEPS:
        inc = incl if "inclusions" in steps else None
        want = _tips.mirror_run(edges, out_off, in_nodes, in_off, steps, 150, geom, inc)
        got = _tips.device_run(scorer, edges, out_off, in_nodes, in_off, steps, 150, geom, inc)
        where = f"{name} {'>'.join(steps)}"
        for st in ("tips", "branches"):
            if st in steps:
                for k, v in want["counts"][st].items():
                    if k != "cc_rounds":
                        assert got["counts"][st][k] == v, (where, st, k, got["counts"][st], want["counts"][st])
        assert _trans.same_records(got["edges"], want["edges"]), where
        assert np.array_equal(got["in_off"], want["in_off"]) and np.array_equal(got["in_nodes"], want["in_nodes"]), where
        assert np.array_equal(got["edges"]["pos4"], edges["pos4"][got["seq"]]), where
        assert _trans.same_records(got["branching"], want["branching"]), where
        assert np.array_equal(got["tips"], want["tips"]), where
        assert len(want["branching"]) > 0, where  # something was removed
        if steps == ("tips",):
            assert want["counts"]["tips"]["n_removed"] > 0 and want["tips"].sum() > 0, where
            assert want["counts"]["tips"]["n_removed"] <= want["counts"]["tips"]["tip_count"], where
        if name == "repeated" and steps == ("branches",):
            assert want["counts"]["branches"]["n_tied_lists"] > 0, where


def _chain_graphs():
    rng = np.random.default_rng(21)
    n = 20000
    yield "chain_ascending", n, np.arange(n - 1), np.arange(1, n)
    p = rng.permutation(n)
    yield "chain_shuffled", n, p[:-1], p[1:]
    c = 4097
    yield "cycle", c, np.arange(c), (np.arange(c) + 1) % c
    lens = rng.integers(1, 201, 300)
    start = np.concatenate([[0], np.cumsum(lens)])
    V = int(start[-1])
    ids = rng.permutation(V)
    s = np.concatenate([ids[start[k]:start[k + 1] - 1] for k in range(300)])
    t = np.concatenate([ids[start[k] + 1:start[k + 1]] for k in range(300)])
    xs, xt = rng.integers(0, V, 100), rng.integers(0, V, 100)  # a few edges across: branches, more components, removals
    ok = xs != xt
    yield "chains_300", V, np.concatenate([s, xs[ok]]), np.concatenate([t, xt[ok]])


CHAINS = list(_chain_graphs())


@pytest.mark.parametrize("ci", range(len(CHAINS)), ids=[c[0] for c in CHAINS])
def test_components(scorer, ci):
    """The labelling on chains as long as a genome is tiled: hop-per-round propagation would need 20 000 rounds on the ascending chain."""
    name, V, v1, v2 = CHAINS[ci]
    edges, out_off, in_nodes, in_off, _ = _trans.shuffled_graph(v1, v2, V, seed=ci + 50)
    geom = np.zeros(V, READ_GEOM_DTYPE)
    want = _tips.mirror_run(edges, out_off, in_nodes, in_off, ("branches",), 0, geom)
    got = _tips.device_run(scorer, edges, out_off, in_nodes, in_off, ("branches",), 0, geom)
    gc, wc = got["counts"]["branches"], want["counts"]["branches"]
    assert gc["n_components"] == wc["n_components"], (name, gc, wc)
    assert gc["cc_rounds"] <= 2 * math.ceil(math.log2(V)) + 2, gc
    assert _trans.same_records(got["branching"], want["branching"]) and _trans.same_records(got["edges"], want["edges"]), name
    if name in ("chain_ascending", "chain_shuffled", "cycle"):
        assert wc["n_components"] == 1 and wc["n_removed"] == 0
    else:
        assert wc["n_components"] > 300 and wc["n_removed"] > 0


def test_branching_edges_feed_fno(scorer):
    """graph_branching_edges() and the cleaned graph handed to the FNO=1 device route give the lines the mirror's give the host route."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fno_bench

    V = 2000
    inp = fno_bench.big_fno1(V, 500, 100, seed=5)
    a, b = _trans.interval_edges(V, 3, seed=8)
    edges, out_off, in_nodes, in_off, _ = _trans.shuffled_graph(a, b, V, seed=60)
    paired = inp.nodes["paired"].astype(bool)
    anyp = paired[edges["v1"].astype(np.int64)] | paired[edges["v2"].astype(np.int64)]
    both = paired[edges["v1"].astype(np.int64)] & paired[edges["v2"].astype(np.int64)]
    rng = np.random.default_rng(9)
    edges["ord"] = np.where(both, np.where(rng.random(edges.size) < 0.5, ord("1"), ord("2")), ord("-"))
    edges["len2"] = np.where(anyp, edges["len2"] + 20, 0)
    edges["len0"] = edges["len1"] + edges["len2"]
    edges["pos2"] = np.where(anyp, rng.integers(0, 9, edges.size), 0)
    geom = np.zeros(V, READ_GEOM_DTYPE)
    geom["len1"], geom["len2"], geom["paired"] = inp.nodes["len1"], inp.nodes["len2"], inp.nodes["paired"]
    steps = ("tips", "branches")
    want = _tips.mirror_run(edges, out_off, in_nodes, in_off, steps, 150, geom)
    got = _tips.device_run(scorer, edges, out_off, in_nodes, in_off, steps, 150, geom)
    assert len(got["branching"]) > 0 and len(got["edges"]) > 0

    def lines(res, route):
        inp.graph_edges, inp.branching_edges = F.edges_from_graph(res["edges"]), F.edges_from_graph(res["branching"])
        os.environ["HC_FNO"] = route
        try:
            return F.find_next_overlaps(inp)
        finally:
            os.environ.pop("HC_FNO", None)

    host_text, host_counts = lines(want, "host")
    assert not F.last_on_device
    dev_text, dev_counts = lines(got, "device")
    assert F.last_device_level > 0
    assert dev_counts == host_counts and dev_text == host_text
    inp.branching_edges = F.edges_from_graph(got["branching"][:0])
    os.environ["HC_FNO"] = "host"
    try:
        without, _ = F.find_next_overlaps(inp)
    finally:
        os.environ.pop("HC_FNO", None)
    assert without != host_text, "the branching edges contribute lines"


def test_refusals_and_reset(scorer):
    """No graph; a resolved graph with tied lists (HC_ERR_STATE, graph untouched); a read index beyond n_reads (HC_ERR_ARG, graph
    untouched); hc_graph_load empties branching_edges and the tip flags."""
    geom = np.zeros(300, READ_GEOM_DTYPE)
    geom["len1"] = 250
    with hc.EdgeScorer(hc.Settings()) as sc:
        for call in (lambda: sc.graph_remove_tips(150, geom), sc.graph_remove_branches, sc.graph_branching_edges, lambda: sc.graph_tip_reads(4)):
            with pytest.raises(hc.HcError) as err:
                call()
            assert err.value.status == -5  # HC_ERR_STATE
    V, m = 300, 40000
    reads, adm = _admitted(1, V, m, 0.0)
    st = hc.Settings(edge_threshold=0.97, flags=FLAG_RESOLVE_ORIENTATIONS | FLAG_IGNORE_INCLUSIONS)
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        sgot = sc.graph_resolve(adm, V, sorted_order=True)
        assert sgot["counts"]["n_tied_lists"] > 0
        for call in (lambda: sc.graph_remove_tips(150, geom), sc.graph_remove_branches):
            with pytest.raises(hc.HcError) as err:
                call()
            assert err.value.status == -5
        still = sc.graph_fetch()
        assert still["edges"].tobytes() == sgot["edges"].tobytes() and np.array_equal(still["in_nodes"], sgot["in_nodes"])
        assert sc.graph_branching_edges().size == 0
    name, edges, out_off, in_nodes, in_off, incl, g5 = _seeded(0)
    scorer.graph_load(edges, out_off, in_nodes, in_off)
    with pytest.raises(hc.HcError) as err:
        scorer.graph_remove_tips(150, g5[: int(edges["read2"].max())])
    assert err.value.status == -1  # HC_ERR_ARG
    still = scorer.graph_fetch()
    assert still["edges"].tobytes() == edges.tobytes() and np.array_equal(still["in_nodes"], in_nodes)
    assert scorer.graph_branching_edges().size == 0 and scorer.graph_tip_reads(len(g5)).sum() == 0
    c = scorer.graph_remove_tips(150, g5)
    assert c["n_removed"] > 0 and scorer.graph_branching_edges().size == c["n_removed"] and scorer.graph_tip_reads(len(g5)).sum() == c["n_tip_reads"]
    scorer.graph_load(edges, out_off, in_nodes, in_off)
    assert scorer.graph_branching_edges().size == 0 and scorer.graph_tip_reads(len(g5)).sum() == 0
