"""hc_host_br_evidence, the host mirror of hc_br_evidence (include/hcsr.h): equal to every recorded reference vector (tests/golden/
branch_evidence.json, made by the reference's own findBranchingEvidence), equal to the Python restatement of src/BranchReduction.cpp:229-743
(tests/_branch_evidence.restate) on seeded and hand-built cases, every status on a case built for it, and the refusals.  No GPU."""
import copy

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import branch_evidence as BR
from tests import _branch_evidence as T

GOLDEN, GOLDEN_FILE = T.golden_cases()
STATUS = T.status_cases()


def test_golden_file_holds_what_the_issue_asks_for():
    cover, need = GOLDEN_FILE["cover"], GOLDEN_FILE["required_cover"]
    assert need == dict(branches=40, missing_inclusion_2=1, missing_inclusion_more=1, missing_inclusion=8, identical=6, cap100=1, both_sides_smaller=10,
                        via_mate1=1, via_mate2=1, via_single=1, reverse_in=1, reverse_out=1, reverse_entry=1, negative_index1=1)
    assert all(cover[k] >= v for k, v in need.items())
    assert "probe with substitutes" in GOLDEN_FILE["provenance"]


@pytest.mark.parametrize("k", range(len(GOLDEN)), ids=[c.name for c, _ in GOLDEN])
def test_mirror_equals_the_reference_on_every_golden_case(k):
    case, want = GOLDEN[k]
    res = T.host_run(case)
    got = T.as_expected(res)
    for table in ("branches", "evidence", "missing"):  # every case whole, every field
        assert got[table] == want[table], table
    T.check_counts(res, want)


@pytest.mark.parametrize("k", range(len(GOLDEN)), ids=[c.name for c, _ in GOLDEN])
def test_restatement_equals_the_reference_on_every_golden_case(k):
    case, want = GOLDEN[k]
    assert T.restate(case) == want


@pytest.mark.parametrize("seed,kw", [(21, {}), (22, dict(reverse=True, bubbles=2)), (23, dict(garbage=4, cap_pair=True)), (24, dict(max_out=6, n_contigs=30)),
                                     (25, dict(n_orig_se=80, n_orig_pe=90, island_step=40, bubbles=3))])
def test_mirror_equals_the_restatement_of_the_cited_lines_on_seeded_cases(seed, kw):
    case = T.make_case(seed, **kw)
    want = T.restate(case)
    res = T.host_run(case)
    assert T.as_expected(res) == want
    T.check_counts(res, want)
    assert res.counts["n_items"] == sum(len(case.dicts[case.vertex_read[v]]) for b in want["branches"] for v in _neighbours(case, b))


def _neighbours(case, b):
    if b["side"]:
        return sorted(v for u, v, _ in case.edges if u == b["node"])
    return sorted(u for u, v, _ in case.edges if v == b["node"])


def test_mirror_equals_the_restatement_of_the_cited_lines_on_fans():
    fans = [dict(k=2, L=1, diffs=[[], [0]], dict_sizes=[1, 1]), dict(k=3, L=63, diffs=[[], [62], []], dict_sizes=[0, 2, 3]),
            dict(k=2, L=64, diffs=[[], [0, 63]], dict_sizes=[5, 5], fwd=0), dict(side="in", k=3, L=65, diffs=[[], [64], [0, 1]], dict_sizes=[4, 4, 4]),
            dict(side="in", k=2, L=129, diffs=[[], list(range(0, 129))], dict_sizes=[6, 6], fwd=0), dict(k=4, L=200, shift=7, diffs=[[], [3], [9], [150]],
                                                                                                     dict_sizes=[3, 3, 3, 3])]
    case = T.fan_case(31, fans)
    want = T.restate(case)
    assert T.as_expected(T.host_run(case)) == want
    assert sum(len(b["diffs"]) > 0 for b in want["branches"]) >= 4  # (the overlap of 1 is below min_overlap_len: a missing inclusion pair)


def test_threads_do_not_change_the_tables():
    case = T.make_case(26, bubbles=2)
    T.assert_same_tables(T.host_run(case, 1), T.host_run(case, 7))


@pytest.mark.parametrize("name", sorted(STATUS))
def test_each_status_on_a_case_built_for_it(name):
    case, statuses = STATUS[name]
    res = T.host_run(case)
    got = {(int(b["node"]), int(b["side"])): int(b["status"]) for b in res.branches if b["status"] != BR.BR_OK}
    assert got == statuses
    assert res.counts["some_failed"] and res.counts["n_failed"] == len(statuses)
    # a failed branch contributes nothing, and the branches beside it are what they are without it
    for b, r in enumerate(res.branches):
        if r["status"] != BR.BR_OK:
            assert r["nb_count"] == 0 and r["diff_count"] == 0 and r["dist"] == 0 and not r["is_false"]
    failed_nodes = {n for n, _ in statuses}
    assert all(int(m["v1"]) not in failed_nodes for m in res.missing_edges)
    assert T.as_expected(res) == T.restate(case)
    base = T.make_case(5, n_contigs=0, n_orig_se=2, n_orig_pe=1, bubbles=1)
    alone = T.as_expected(T.host_run(base))
    both = T.as_expected(res)
    assert [b for b in both["branches"] if b["node"] < base.n_vertices] == alone["branches"]
    assert {k: v for k, v in both["evidence"].items() if max(k) < base.n_vertices} == alone["evidence"] and alone["evidence"]


def test_refusals():
    case = T.make_case(27, n_contigs=12)
    T.host_run(case)
    for change, what in ((dict(se_count=case.se_count + 1), "se_count"), (dict(pe_count=case.pe_count + 1), "se_count"),
                         (dict(original_readcount=1 << 31), "original_readcount")):
        c = copy.deepcopy(case)
        for k, v in change.items():
            setattr(c, k, v)
        with pytest.raises(N.HcError, match=what):  # the assert of src/ViralQuasispecies.cpp:341
            T.host_run(c)
    c = copy.deepcopy(case)
    c.vertex_read[3] = len(c.seqs)
    c.dicts.append([])  # (the dict has one read more, the store does not)
    with pytest.raises((N.HcError, ValueError)):
        T.host_run(c)
    # a neighbour's record that names a read outside the store
    from haploconduct_amd import host

    g = case.graph()
    deg = np.diff(g["out_off"].astype(np.int64))
    u = int(np.argmax(deg > 1))
    g["edges"]["read2"][int(g["out_off"][u])] = len(case.seqs) + 5
    off, entries = case.dict_arrays()
    ob, oo = case.original_arrays()
    with pytest.raises(N.HcError, match="no read of the store"):
        host.br_evidence(g, case.reads(), off, entries, ob, oo, case.vertex_read, case.vertex_fwd, case.settings())

    # ... also where a paired neighbour comes first in the list: the arguments are checked ahead of any status
    case, g = T.paired_then_bad_read()
    off, entries = case.dict_arrays()
    ob, oo = case.original_arrays()
    with pytest.raises(N.HcError, match="no read of the store"):
        host.br_evidence(g, case.reads(), off, entries, ob, oo, case.vertex_read, case.vertex_fwd, case.settings())


def test_an_empty_graph_has_no_branches():
    case = T.Case("empty", ["ACGT"], [0], [1], [], [[]], ["ACGT"], 1, 0, 1)
    res = T.host_run(case)
    assert res.counts["n_branches"] == 0 and res.ev_off.tolist() == [0] and not res.counts["some_failed"]
