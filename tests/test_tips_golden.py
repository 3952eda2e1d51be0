"""The host mirror of OverlapGraph::removeTips / removeBranches (hc_host_graph_remove_tips / _remove_branches) against the
reference's own results (tests/golden/tips_branches.json, make_golden_tips.py): records, list order, adj_in, the order of
branching_edges, tip flags and counters of every variant; and the coverage conditions the generator asserted, on the file."""
import numpy as np
import pytest

from tests import _tips, _trans

CASES = _tips.load_cases()


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_mirror_equals_reference(name):
    case = next(c for c in CASES if c["name"] == name)
    V = case["V"]
    recs = _tips.golden_records(case["edges_in"])
    geom = _tips.read_geom(case["reads"])
    edges, out_off, in_nodes, in_off = _trans.csr_from_inserts(recs, V)
    for vname, steps in _tips.VARIANTS.items():
        var = case["variants"][vname]
        got = _tips.mirror_run(edges, out_off, in_nodes, in_off, steps, case["max_tip_len"], geom)
        where = f"{name} {vname}"
        assert _trans.same_records(got["edges"], recs[var["out"]]), where
        assert got["in_off"].tolist() == var["in_off"] and got["in_nodes"].tolist() == var["in_nodes"], where
        assert _trans.same_records(got["branching"], recs[var["branching"]]), where
        assert got["tips"].tolist() == var["tip_reads"], where
        _tips.check_counts(got["counts"], var, where)


def test_golden_file_covers_what_it_should():
    """At least one case each: fewer pairs removed than tips counted; tips counted and nothing removed (alltips); several
    components of which one is a cycle; a tied list; a read that is not a vertex; all of max_tip_len 0 / 150 / in between."""
    by = {c["name"]: c for c in CASES}
    tips = [c["variants"]["tips"] for c in CASES]
    assert any(0 < len(t["branching"]) < t["tip_count"] for t in tips)
    assert any(t["tip_count"] > 0 and not t["branching"] for t in tips)
    assert any(c["variants"]["branches"]["n_tied_lists"] > 0 for c in CASES)
    cyc = by["cycle"]["variants"]["branches"]
    kept = [by["cycle"]["edges_in"][k][:2] for k in cyc["out"]]
    assert cyc["n_components"] > 1 and all([i, (i + 1) % 7] in kept for i in range(7))
    assert any(e[0] != e[2] or e[1] != e[3] for e in by["duplicates"]["edges_in"])
    assert any(e[4] + e[5] < 0 for c in CASES for e in c["edges_in"])
    assert {c["max_tip_len"] for c in CASES} >= {0, 150, 1, 40}
    assert by["empty"]["edges_in"] == [] and by["empty"]["variants"]["branches"]["n_components"] == by["empty"]["V"]
    assert all(max(c["V"] for c in CASES) <= 200 for _ in [0])
    # every branch of Edge::ext_len: the four read-type combinations with ord 1 / 2 / -, both ori2
    seen = set()
    for c in CASES:
        for e in c["edges_in"]:
            seen.add((c["reads"][e[2]][2], c["reads"][e[3]][2], chr(e[10]), e[9]))
    assert seen >= {(a, b, o, r) for a in (0, 1) for b in (0, 1) for o in "12-" for r in (0, 1)}
