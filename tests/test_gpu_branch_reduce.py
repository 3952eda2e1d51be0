"""hc_br_evidence -> hc_br_reduce on the device against hc_host_br_evidence -> hc_host_br_reduce, for equality: the hc_br_reduce_fetch tables, the
reduced graph by hc_graph_fetch, branching_edges record for record, then graph.txt and hc_graph_merge_pairs on the reduced device graph against
the same on the mirror's graph loaded afresh.  Graphs come through hc_graph_load, the dict through hc_sr_originals_load, the reads through
set_reads with keeping on.  The shapes are the smallest at which each kernel can go wrong: evidence lists around a wave and one of 5 000 ids,
ids shared inside a component and between components, components of 1 to 300 edges, 20 000 components, ids at 2 * original_readcount - 1 with
original_readcount small and at 2^31 - 1, in-lists around a wave for the ballot that finds the adj_in entry.

The golden cases of tests/golden/branch_reduce.json are tables, which the device call cannot be given; the evidence golden cases stand in for
them here.  The device call shares find_components / decide / run_chain with the mirror (one source), so equality with the mirror checks on
its own the unique counts, the general rule, the pairs' records and the edit; the shared part is pinned by the golden cases on the host.

Not reachable through hc_br_evidence, and therefore covered on the host alone (tests/test_branch_reduce_host.py): a removed pair whose (u, v)
repeats (a repeated neighbour fails its branch, HC_BR_REPEATED_NEIGHBOUR), a component edge without a row, an edge in two components — so the
device call's fetch of the whole evidence tables for such components runs in no test, only the mirror's routines it would call —, and an id
in ALL lists of a component: the lists of a component's edges at one branch belong to neighbours that differ pairwise at a position of the
diff list, an id is evidence only where its read covers a diff position and agrees there (checkReadEvidence), and a read that covers the
position where two neighbours differ cannot agree with both (the mirror's golden case double4_shared_ids has such an id)."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import branch_evidence as BR
from haploconduct_amd import host
from tests import _branch_evidence as E
from tests import _branch_reduce as T

pytestmark = pytest.mark.gpu

TABLE = {d: (2 if d < 300 else 4) for d in range(100, 1000)}


@pytest.fixture(scope="module")
def scorer():
    with hc.EdgeScorer(hc.Settings(edge_threshold=0.97, min_overlap_len=10)) as sc:
        sc.sr_keep_device(True)
        yield sc


def load(sc, case, g):
    sc.set_reads(case.reads())
    sc.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
    sc.sr_originals_load(*case.dict_arrays())
    sc.br_set_original_reads(*case.original_arrays())


def mirror_run(case, g, settings):
    off, entries = case.dict_arrays()
    ob, oo = case.original_arrays()
    ev = host.br_evidence(g, case.reads(), off, entries, ob, oo, case.vertex_read, case.vertex_fwd, case.settings())
    return ev, host.br_reduce(g, case.reads(), ev, settings)


def check(sc, case, g=None, thresholds=TABLE, careful=0, diploid=1, downstream=True):
    """the device chain against the mirror's; returns the device's BranchReduction"""
    g = case.graph() if g is None else g
    settings = BR.reduce_settings(thresholds, careful=careful, diploid=diploid)
    ev, mirror = mirror_run(case, g, settings)
    load(sc, case, g)
    cn = sc.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    assert cn["n_ev_ids"] == ev.counts["n_ev_ids"] and cn["n_branches"] == ev.counts["n_branches"]
    counts = sc.br_reduce(settings)
    dev = sc.br_reduce_fetch()
    assert counts["ms_device"] >= 0 and counts["ms_host_walk"] >= 0 and counts["ms_copy"] >= 0
    dg = sc.graph_fetch()
    T.assert_same((dev, dg, sc.graph_branching_edges()), mirror)
    assert dev.counts["n_removed"] == g["edges"].size - dg["edges"].size
    if downstream:
        text, tc = sc.graph_write_text("cliques", edge_threshold=0.9)
        pairs = sc.graph_merge_pairs()
        mg = mirror[1]
        sc.graph_load(mg["edges"], mg["out_off"], mg["in_nodes"], mg["in_off"])
        text2, tc2 = sc.graph_write_text("cliques", edge_threshold=0.9)
        assert text == text2 and tc["n_bytes"] == tc2["n_bytes"] and tc["status"] == tc2["status"]
        assert np.array_equal(pairs, sc.graph_merge_pairs())
    return dev


GOLDEN_EV, _ = E.golden_cases()


@pytest.mark.parametrize("careful,diploid", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("k", range(len(GOLDEN_EV)), ids=[c.name for c, _ in GOLDEN_EV])
def test_the_evidence_golden_cases_reduced(scorer, k, careful, diploid):
    case, _ = GOLDEN_EV[k]
    g = case.graph()
    g["edges"]["len0"] = np.where(np.arange(g["edges"].size) % 3 == 0, 99, 100)  # both sides of :818
    dev = check(scorer, case, g, thresholds={d: 1 + d % 3 for d in range(100, 2000)}, careful=careful, diploid=diploid)
    assert dev.counts["n_components"] + dev.counts["n_false_dropped"] > 0  # ("wide" holds false branches only)
    if not diploid:
        assert dev.counts["n_host_finished"] == 0 and not dev.components["host_finished"].any()


@pytest.mark.parametrize("seed", [201, 202, 203])
@pytest.mark.parametrize("careful,diploid", [(0, 1), (1, 0), (1, 1)])
def test_seeded_graphs_with_bubbles(scorer, seed, careful, diploid):
    case = E.make_case(seed, bubbles=6, max_out=4)
    dev = check(scorer, case, thresholds={d: 1 + (d // 7) % 2 for d in range(100, 3000) if d % 11}, careful=careful, diploid=diploid)
    assert dev.counts["n_components"] > 0
    if not diploid:
        assert dev.counts["n_host_finished"] == 0 and not dev.components["host_finished"].any()


def test_evidence_lists_of_0_1_63_64_65_and_5000_ids(scorer):
    case, g = T.evidence_fans(301, [dict(sizes=[0, 1, 63, 64, 65, 5000]), dict(sizes=[64, 0]), dict(sizes=[1, 1])])
    dev = check(scorer, case, g, thresholds={d: 64 for d in range(100, 400)})
    assert sorted(dev.comp_unique.tolist()) == [0, 0, 1, 1, 1, 63, 64, 64, 65, 5000] and dev.counts["n_items_sorted"] == 5259
    assert dev.counts["n_removed"] == 6 and dev.counts["n_kept"] == 2


def test_an_id_shared_by_2_by_3_and_by_all_but_one_list_and_one_id_in_two_components(scorer):
    fan = dict(sizes=[3, 3, 3, 3, 3], shared=[(1, [0, 2]), (2, [0, 1, 3]), (3, [0, 1, 2, 4])])
    case, g = T.evidence_fans(302, [fan, dict(fan, common=("own", 0), same_as=0), dict(sizes=[2, 2])])
    dev = check(scorer, case, g, thresholds={d: 3 for d in range(100, 400)}, diploid=0)
    assert sorted(dev.comp_unique.tolist()) == [2, 2] + [3] * 10  # shared ids count nowhere
    assert dev.counts["n_items_sorted"] == 2 * (15 + 2 + 3 + 4) + 4 and dev.counts["n_removed"] == 2


@pytest.mark.parametrize("k", [2, 4, 64, 300])
def test_components_of_2_4_64_and_300_edges(scorer, k):
    sizes = [(j * 5) % 4 for j in range(k)]
    case, g = T.evidence_fans(303 + k, [dict(sizes=sizes, L=max(40, k + 20)), dict(sizes=[1, 2])])
    dev = check(scorer, case, g, thresholds={d: 2 for d in range(100, 1000)}, diploid=0, downstream=k < 300)
    assert sorted(dev.components["edge_count"].tolist()) == sorted([2, k])
    assert dev.counts["n_removed"] == sum(1 for s in sizes if s < 2) + 1


@pytest.mark.parametrize("min_evidence", [0, 1])
def test_a_component_of_one_edge(scorer, min_evidence):
    """an out-branch of three neighbours of which two end more than min_overlap_len before the third begins: both leave final_branch as
    missing inclusion pairs (:328-335), the branch keeps one neighbour and is a listed component of one edge.  Its evidence is empty (every
    diff position lies in front of the neighbour that stays), so min_evidence 1 removes it and 0 keeps it."""
    rng = np.random.default_rng(501)
    a, b, b2, c = E.random_seq(rng, 80), E.random_seq(rng, 30), E.random_seq(rng, 30), E.random_seq(rng, 60)
    case = E.Case("one_edge", [a, b, b2, c], [0, 1, 2, 3], [1] * 4, [(0, 1, 5), (0, 2, 7), (0, 3, 40)], [[]] * 4, ["ACGT"], 1, 0, 1)
    dev = check(scorer, case, thresholds={d: min_evidence for d in range(100, 1000)})
    assert dev.components["edge_count"].tolist() == [1] and dev.comp_edge.tolist() == [[0, 3]]
    assert dev.removed.tolist() == ([[0, 3]] if min_evidence else [])


def test_twenty_thousand_components(scorer):
    fans = [dict(sizes=[1 + i % 2, (i // 2) % 3], L=24) for i in range(20000)]
    case, g = T.evidence_fans(304, fans)
    dev = check(scorer, case, g, thresholds={d: 2 for d in range(100, 400)}, downstream=False)
    assert dev.counts["n_components"] == 20000 and dev.counts["n_host_finished"] == 0


@pytest.mark.parametrize("orc", [None, 2 ** 31 - 1])
def test_ids_at_twice_the_original_readcount_less_one(scorer, orc):
    # all originals are pairs: se = 0, pe = 6, ids of /1 mates 0 .. 5, so the joint ids are orc + 0 .. orc + 5
    case, g = T.evidence_fans(305, [dict(sizes=[3, 3], paired=3)], original_readcount=6 if orc is None else orc)
    assert case.se_count == 0 and case.pe_count == 6
    dev = check(scorer, case, g, thresholds={d: 3 for d in range(100, 400)})
    assert dev.comp_unique.tolist() == [3, 3] and dev.counts["n_removed"] == 0
    load(scorer, case, g)
    scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    ids = scorer.br_evidence_fetch().ev_ids
    assert int(ids.max()) == (11 if orc is None else orc + 5)  # 2 * 6 - 1: the largest id the key's id field must hold


@pytest.mark.parametrize("k", [63, 64, 65, 200])
def test_a_removed_pair_in_lists_of_63_64_65_and_200_records(scorer, k):
    """an out-branch and an in-branch of k neighbours: the pair's record is found by bisection over k records, its adj_in entry by the
    ballot over an in-list of k entries (the in-branch) — all removed under a threshold nothing meets, some under a low one"""
    def diffs(L):
        return [[]] + [[j] for j in range(1, k)]  # every neighbour differs from neighbour 0 at a position of its own: no false branch

    L = k + 61
    fans = [dict(k=k, L=L, diffs=diffs(L), dict_sizes=[j % 3 for j in range(k)]), dict(k=k, L=L, diffs=diffs(L), dict_sizes=[(j + 1) % 3 for j in range(k)], side="in")]
    for min_ev in (1, 50):
        case = E.fan_case(400 + k, fans)
        g = case.graph()
        rng = np.random.default_rng(k)
        for v in range(case.n_vertices):  # adj_in in another order than ascending: the FIRST entry u is found where it lies
            a, b = int(g["in_off"][v]), int(g["in_off"][v + 1])
            g["in_nodes"][a:b] = rng.permutation(g["in_nodes"][a:b])
        dev = check(scorer, case, g, thresholds={d: min_ev for d in range(100, 1000)}, diploid=0, downstream=min_ev == 1)
        if min_ev == 50:
            assert dev.counts["n_removed"] == 2 * k


def test_a_typical_double_branch_is_finished_by_the_host_under_diploid_only(scorer):
    case = E.make_case(5, n_contigs=0, n_orig_se=2, n_orig_pe=1, bubbles=1)  # one bubble: 0 -> {1, 2} -> 3
    for diploid in (1, 0):
        dev = check(scorer, case, thresholds={d: 1 for d in range(100, 1000)}, diploid=diploid)
        typical = [i for i, c in enumerate(dev.components) if c["edge_count"] in (3, 4)]
        assert dev.counts["n_host_finished"] == (len(typical) if diploid else 0)
        assert all((dev.components[i]["host_finished"] == BR.RED_HOST_DIPLOID) == bool(diploid) for i in typical)


def test_state_errors(scorer):
    case, g = T.evidence_fans(306, [dict(sizes=[2, 0])])
    st = BR.reduce_settings({d: 1 for d in range(100, 400)})

    def status(call):
        with pytest.raises(N.HcError) as e:
            call()
        return e.value.status

    load(scorer, case, g)
    assert status(lambda: scorer.br_reduce(st)) == -5  # no hc_br_evidence since the graph was loaded
    scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    assert status(lambda: scorer.br_reduce(BR.reduce_settings({}))) == -1  # an empty table: nothing is spent
    E_before = scorer.graph_fetch()["edges"].size
    assert scorer.br_reduce(st)["n_removed"] == 1
    assert scorer.graph_fetch()["edges"].size == E_before - 1
    assert status(lambda: scorer.br_reduce(st)) == -5           # spent
    assert status(lambda: scorer.br_evidence_fetch()) == -5     # spent
    assert scorer.br_reduce_fetch().removed.tolist() == [[0, 2]]
    # the tables go with the graph, and a cleaning call between the two halves is refused
    scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    scorer.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
    assert status(lambda: scorer.br_reduce(st)) == -5 and status(lambda: scorer.br_reduce_fetch()) == -5
    scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    scorer.graph_remove_branches()
    assert status(lambda: scorer.br_reduce(st)) == -5
