"""The host mirror of OverlapGraph::removeInclusions + removeTransitiveEdges against the reference's own results
(tests/golden/trans_edges.json, make_golden_trans.py): records in list order, adj_in, edge_count, inclusion groups and
transitive_count, for every case and variant."""
import numpy as np
import pytest

from tests import _trans

CASES = _trans.load_cases()
IDS = [(c["name"], i) for c in CASES for i in range(len(c["variants"]))]


@pytest.mark.parametrize("name,vi", IDS, ids=[f"{n}-{i}" for n, i in IDS])
def test_mirror_equals_reference(name, vi):
    case = next(c for c in CASES if c["name"] == name)
    var = case["variants"][vi]
    V = case["V"]
    recs = _trans.golden_records(case["edges_in"])
    edges, out_off, in_nodes, in_off = _trans.csr_from_inserts(recs, V)
    m = _trans.Mirror(edges, out_off, in_nodes, in_off, case["incl"] if var["inclusions"] else None)
    if var["inclusions"]:
        goff, gedges = m.remove_inclusions()
        assert goff.tolist() == var["group_off"]
        assert _trans.same_records(gedges, recs[var["group_edges"]])
    counts = m.remove_transitive(var["remove_trans"], var["branch_reduction"])
    out, ioff, inodes = m.result()
    assert counts["edges_after"] == var["edge_count"]
    assert counts["transitive_count"] == var["transitive_count"]
    assert _trans.same_records(out, recs[var["out"]])
    assert np.array_equal(np.bincount(out["v1"].astype(np.int64), minlength=V), np.diff(var["out_off"]))
    assert ioff.tolist() == var["in_off"] and inodes.tolist() == var["in_nodes"]


def test_cases_cover_both_branches_and_ties():
    """The golden cases reach both removal branches and hold repeated targets in lists of more than 16 entries."""
    seen, tied = set(), 0
    for case in CASES:
        recs = _trans.golden_records(case["edges_in"])
        edges, out_off, in_nodes, in_off = _trans.csr_from_inserts(recs, case["V"])
        for var in case["variants"]:
            m = _trans.Mirror(edges, out_off, in_nodes, in_off, case["incl"] if var["inclusions"] else None)
            if var["inclusions"]:
                m.remove_inclusions()
            c = m.remove_transitive(var["remove_trans"], var["branch_reduction"])
            seen.add(c["rebuilt"])
            tied += c["n_tied_lists"]
    assert seen == {0, 1} and tied > 0
