"""hc_host_br_reduce, the host mirror of the second half of BranchReduction::readBasedBranchReduction (reference src/BranchReduction.cpp:82-227,
:745-1272), against tests/golden/branch_reduce.json — what a probe around the reference's own lines computed — whole, case by case; the Python
restatement of tests/_branch_reduce.py against the same file with the recorded unordered_map orders, and with ascending orders where it must
DIFFER; the library's own unordered_map order against the recorded one; hc_host_br_parse_thresholds against the table the reference's
scripts/min_ev_table.py wrote.  No GPU."""
import os

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import branch_evidence as BR
from tests import _branch_reduce as T

GOLDEN, DATA = T.golden()
HERE = os.path.dirname(os.path.abspath(__file__))


def expected(want):
    return dict(components=[(d, [tuple(p) for p in c]) for d, c in want["components"]], removed=[tuple(p) for p in want["removed"]],
                adj_out=[[tuple(x) for x in l] for l in want["adj_out"]], adj_in=want["adj_in"], branching=[tuple(p) for p in want["branching"]])


def without_outcomes(d):
    d = dict(d)
    d.pop("outcomes")
    return d


def test_the_library_iterates_an_unordered_map_as_the_recorded_standard_library_does():
    got = BR.map_order(41)
    assert got == DATA["unordered_map_order_0_40"], (
        "std::unordered_map< unsigned long, bool > filled with 0..40 iterates in another order than the probe's did: the library is built against a "
        "standard library other than the libstdc++ the golden file was recorded with (" + DATA["provenance"] + "); hc_br_reduce's component "
        "order, dist and --careful chain follow the reference only under the reference's standard library")
    assert got != sorted(got)


@pytest.mark.parametrize("k", range(len(GOLDEN)), ids=[c.name for c, _, _ in GOLDEN])
def test_mirror_equals_the_reference_on_every_golden_case(k):
    case, want, _ = GOLDEN[k]
    red, graph, branching = T.host_run(case)
    assert without_outcomes(T.as_expected(red, graph, branching)) == expected(want)
    assert red.counts["n_removed"] == len(want["removed"]) and red.counts["n_missing_appended"] == case.n_missing
    assert red.counts["n_components"] == len(want["components"])


@pytest.mark.parametrize("k", range(len(GOLDEN)), ids=[c.name for c, _, _ in GOLDEN])
def test_restatement_with_the_recorded_orders_equals_the_reference_and_the_mirror(k):
    case, want, orders = GOLDEN[k]
    mine = T.restate(case, T.recorded_order(orders))
    assert without_outcomes(mine) == expected(want)
    red, graph, branching = T.host_run(case)
    assert T.as_expected(red, graph, branching) == mine  # the outcomes too


def test_ascending_order_differs_on_the_rehash_case():
    case, want, orders = next(g for g in GOLDEN if g[0].name == "rehash")
    in_order = orders[0]
    assert len(in_order) >= 30 and in_order[0] not in (min(in_order), max(in_order))
    assert in_order.index(9) < in_order.index(5)  # libstdc++ reaches the in-branch with the larger dist first
    asc = T.restate(case, T.ascending)
    ref = expected(want)
    assert without_outcomes(asc) != ref
    d_asc = {tuple(c): d for d, c in asc["components"]}
    d_ref = {tuple(c): d for d, c in ref["components"]}
    comp = ((36, 5), (36, 9), (37, 5), (37, 9))
    assert d_asc[comp] == 120 and d_ref[comp] == 180  # either side of the table's step at 150
    assert set(comp) <= set(ref["removed"]) and not set(comp) & set(asc["removed"])


def test_counts_outcomes_and_host_finished_marks():
    by = {c.name: c for c, _, _ in GOLDEN}
    red, _, _ = T.host_run(by["no_threshold"])
    assert red.components["outcome"].tolist() == [BR.RED_NO_THRESHOLD] and red.components["min_evidence"].tolist() == [-1]
    assert red.counts["n_no_threshold"] == 1 and red.counts["n_removed"] == 2 and red.comp_unique.tolist() == [0, 0]
    red, _, _ = T.host_run(by["shared_vertex_c1_33"])
    assert sorted(red.components["outcome"].tolist()) == [BR.RED_KEPT, BR.RED_CAREFUL] and red.counts["n_careful_dropped"] == 1
    red, _, _ = T.host_run(by["false_inside"])
    assert red.counts["n_false_dropped"] == 1 and red.counts["n_components"] == 0 and red.counts["n_removed"] == 4
    red, _, _ = T.host_run(by["double4_shared_ids"])
    assert red.comp_unique.tolist() == [3, 3, 3, 3] and red.counts["n_items_sorted"] == 12 + 2 + 3 + 4
    assert red.components["host_finished"].tolist() == [BR.RED_HOST_DIPLOID] and red.counts["n_host_finished"] == 1
    red, _, _ = T.host_run(by["double4_2255_gen"])
    assert red.components["host_finished"].tolist() == [0] and red.counts["n_host_finished"] == 0


def test_a_component_edge_without_a_row_and_an_edge_in_two_components():
    # :1029-1031: (0, 2) has no key; evidence_status is one short, index 0 then belongs to (0, 2) whose at() throws
    case = T.build("no_row", 3, [(0, 1), (0, 2)], counts={(0, 1): 3, (0, 2): 3})
    del case.evidence[(0, 1)]
    with pytest.raises(N.HcError) as e:
        T.host_run(case)
    assert e.value.status == -1 and "at()" in str(e.value)
    with pytest.raises(T.Ends):
        T.restate(case)
    # the last edge's key is missing and the edge in front of it is empty: no index is reached whose list is missing
    case = T.build("no_row_tail", 4, [(0, 1), (0, 2), (0, 3)], counts={(0, 1): 3, (0, 2): 0, (0, 3): 3})
    del case.evidence[(0, 3)]
    red, graph, branching = T.host_run(case)
    assert T.as_expected(red, graph, branching) == T.restate(case, order=lambda keys: BRorder(keys, case.n_vertices))
    assert red.components["host_finished"].tolist() == [BR.RED_HOST_NO_ROW] and red.comp_unique.tolist() == [3, 0, 0]
    # (an edge in two components cannot be built from any tables: the walk that reaches the branch of one end reaches the other's, see
    # include/hcsr.h; HC_BR_RED_HOST_SHARED_EDGE is therefore 0 everywhere, which the counts of every case above and below confirm)


def BRorder(keys, V):
    """the library's unordered_map order for small key sets that never rehash past 13 buckets: reverse insertion order (every key lands in a
    bucket of its own at the front of the list) — enough for the hand-made cases of this file, which have at most four keys per map"""
    assert len(keys) <= 4
    return list(reversed(keys))


def test_parse_thresholds_reads_the_table_min_ev_table_py_wrote():
    text = open(os.path.join(HERE, "golden", "evidence_threshold_table.tsv")).read()
    got = BR.parse_thresholds(text)
    want = [(int(f[0]), int(f[2])) for f in (l.split("\t") for l in text.split("\n") if l and not l.startswith("#"))]
    assert len(want) > 100 and [tuple(x) for x in got.tolist()] == sorted(want)
    assert got["dist"].tolist() == list(range(1, len(want) + 1))


def test_parse_thresholds_comments_empty_lines_later_lines_and_bad_lines():
    got = BR.parse_thresholds("# a comment\n\n100\t7\t3\n101\t8\t4\n#x\t1\n100\t9\t5\n102\t1\t 6x\n")
    assert [tuple(x) for x in got.tolist()] == [(100, 5), (101, 4), (102, 6)]  # the later line wins; stoi stops at the x
    assert BR.parse_thresholds("").size == 0 and BR.parse_thresholds("# only\n\n").size == 0
    assert [tuple(x) for x in BR.parse_thresholds("-3\t0\t+2").tolist()] == [(-3, 2)]  # no newline at the end
    for text, line in (("100\t1\t2\nabc\t1\t2\n", 2), ("# c\n\n100\t1\tx\n", 3), ("100\t1\t2\n101\t1\t99999999999\n", 2), ("\t1\t2\n", 1)):
        with pytest.raises(N.HcError) as e:
            BR.parse_thresholds(text)
        assert e.value.status == -1 and e.value.bad_line == line, text
    # a fourth field stays in the reference's stringstream and lands in front of the next line's dist (:144, :152)
    with pytest.raises(N.HcError) as e:
        BR.parse_thresholds("100\t1\t2\tx\n101\t1\t3\n")
    assert e.value.bad_line == 2
    assert [tuple(x) for x in BR.parse_thresholds("100\t1\t2\t\n101\t1\t3\n").tolist()] == [(100, 2), (101, 3)]
    # two fields: the third getline fails and tmp keeps the second field
    assert [tuple(x) for x in BR.parse_thresholds("100\t7\n").tolist()] == [(100, 7)]


def test_refusals():
    case = GOLDEN[0][0]
    g, reads, ev = case.graph(), case.reads(), case.tables()
    with pytest.raises(N.HcError) as e:
        BR.host_reduce(g, reads, ev, BR.reduce_settings({}))
    assert e.value.status == -1 and "157" in str(e.value)
    bad = T.build("not_in_graph", 3, [(0, 1), (0, 2)])
    bad.branches = [(0, T.OUT, 100, 0, [1, 2]), (1, T.OUT, 100, 0, [0, 2])]
    with pytest.raises(N.HcError) as e:
        T.host_run(bad)
    assert e.value.status == -1


@pytest.mark.parametrize("seed", range(6))
def test_mirror_equals_the_restatement_on_seeded_graphs_without_ties_in_the_order(seed):
    """random small graphs whose maps hold at most one in-branch and one out-branch component start each would need the library's order; here
    every component is reached from a single start whatever the order, because the graph is ONE double-branch ladder: the restatement with
    any order equals the mirror"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 5))
    # out-nodes 0 .. n - 1, in-nodes n .. 2n - 1, a ladder: i -> n + i and i -> n + i + 1
    edges = sorted({(i, n + i) for i in range(n)} | {(i, n + i + 1) for i in range(n - 1)} | {(n - 1, n)})
    counts = {e: int(rng.integers(0, 5)) for e in edges}
    case = T.build(f"ladder{seed}", 2 * n, edges, counts=counts, diploid=0, careful=int(seed % 2),
                   shared=[(0, [edges[0], edges[-1]]), (1, list(edges))])
    red, graph, branching = T.host_run(case)
    mine = T.restate(case, T.ascending)
    assert red.counts["n_components"] == 1
    got = T.as_expected(red, graph, branching)
    assert got["removed"] == mine["removed"] and got["adj_out"] == mine["adj_out"] and got["adj_in"] == mine["adj_in"] and got["branching"] == mine["branching"]
    assert got["components"][0][1] == mine["components"][0][1]
