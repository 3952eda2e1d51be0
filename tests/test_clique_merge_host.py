"""The host mirror of the clique merge (include/hcsr.h: hc_host_sr_clique_merge_layouts, hc_host_sr_clique_filter) against the reference's own
constructSuperread for cliques of any size (tests/golden/clique_merge.json: sort_vertices, filter_subreads with its std::sort, consensus and
calcSubreadInfo, genuine), against hc_host_sr_edge_merge_layouts on cliques of two, its refusals, and the shared group rule of
host/SrCliqueFilter.h against reversed orders inside the endpos groups."""
import ctypes as C

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR
from haploconduct_amd import host as H

from tests import _clique_merge as CM
from tests import _edge_merge as EM


@pytest.fixture(scope="module")
def golden():
    doc = CM.load_golden()
    return doc, CM.golden_graph(doc)


def _mirror(doc, graph, cliques, m, ec, ret=None):
    e, out_off, reads = graph
    off, nodes = SR.clique_csr([q["clique"] for q in cliques])
    return SR.host_clique_merge_layouts(e, out_off, reads, off, nodes, doc["vertex_read"], doc["vertex_fwd"],
                                        SR.make_settings(min_clique_size=m, error_correction=bool(ec)), ret)


def test_golden_holds_what_it_must():
    doc = CM.load_golden()
    sizes = {(q["m"], len(q["clique"])) for q in doc["cliques"]}
    assert {(m, k) for m in CM.MS for k in (3 * m, 3 * m + 1)} <= sizes
    assert {q["type"] for q in doc["cliques"]} == {"s", "p"}
    assert any(len(lst) > 16 and not all(e[5] for e in lst) for q in doc["cliques"] for lst in q["lists"])
    assert any(t == -1 for q in doc["cliques"] for t in q["trim"][:len(q["lists"])])


def test_mirror_equals_the_reference_on_every_golden_clique(golden):
    """Full lists, sorted vertices, member_used and, given the reference's trim positions, the subread infos."""
    doc, graph = golden
    n = 0
    for (m, ec), cliques in sorted(CM.golden_groups(doc).items()):
        want = CM.golden_arrays(cliques)
        got = _mirror(doc, graph, cliques, m, ec, ret=want[7])
        CM.assert_equal_layouts(got, want, f"m={m} ec={ec}")
        filtered = np.asarray([len(q["clique"]) > 3 * m for q in cliques for _ in q["lists"]])
        assert np.array_equal(got.layout_filter != SR.SR_FILTER_NONE, filtered)
        assert got.n_filtered_layouts == int(filtered.sum())
        assert got.n_host_filters == int((got.layout_filter == SR.SR_FILTER_HOST).sum())
        n += len(cliques)
    assert n == len(doc["cliques"]) >= 100


def test_cliques_of_two_equal_the_edge_merge_mirror():
    """Every pair of the edge-merge golden file and the planted failing pairs: statuses, layouts, members and subread infos."""
    for case in EM.load_cases() + [None]:
        if case is None:
            case, pairs, _ = EM.planted()
        else:
            pairs = [p["pair"] for p in case["pairs"]]
        e, out_off, _, _ = EM.csr(case["V"], case["edges_in"])
        reads = EM.random_reads(case["reads"], 4)
        st = SR.make_settings(min_clique_size=2)
        a = SR.host_edge_merge_layouts(e, out_off, reads, pairs, case["vertex_read"], case["vertex_fwd"], st)
        ret = np.arange(a.layouts.size, dtype=np.int32) % 7 - 1
        a = SR.host_edge_merge_layouts(e, out_off, reads, pairs, case["vertex_read"], case["vertex_fwd"], st, ret)
        off, nodes = SR.clique_csr(pairs)
        b = SR.host_clique_merge_layouts(e, out_off, reads, off, nodes, case["vertex_read"], case["vertex_fwd"], st, ret)
        assert np.array_equal(a.pair_status, b.clique_status)
        assert np.array_equal(a.first_layout, b.first_layout) and np.array_equal(a.layouts, b.layouts) and np.array_equal(a.members, b.members)
        assert np.array_equal(a.subreads.reshape(-1), b.subreads)
        assert b.member_used.all() and (b.layout_filter == SR.SR_FILTER_NONE).all()


def test_seeded_cliques_meet_the_device_test_preconditions():
    """What tests/test_gpu_clique_merge.py relies on, on the mirror's output."""
    g = CM.seeded_cliques()
    e, out_off, _, _ = EM.csr(g["V"], g["rows"])
    off, nodes = SR.clique_csr(g["cliques"])
    st = SR.make_settings(min_clique_size=g["m"])
    lay = SR.host_clique_merge_layouts(e, out_off, g["reads"], off, nodes, g["vertex_read"], g["vertex_fwd"], st)
    assert np.array_equal(lay.clique_status, g["want_status"])
    assert 140 <= len(g["cliques"]) <= 170 and 500 <= g["V"] <= 1500
    assert (lay.clique_status == SR.SR_EDGE_OK).mean() >= 0.9
    assert {SR.SR_CLIQUE_TOO_SMALL, SR.SR_CLIQUE_REPEATED_VERTEX, SR.SR_EDGE_BAD_VERTEX, SR.SR_EDGE_NO_EDGE} <= set(lay.clique_status.tolist())
    f = lay.layout_filter
    assert (f != SR.SR_FILTER_NONE).sum() >= 40
    assert ((f == SR.SR_FILTER_GROUPS) | (f == SR.SR_FILTER_STABLE)).sum() >= (f != SR.SR_FILTER_NONE).sum() / 2
    assert (f == SR.SR_FILTER_HOST).sum() >= 10
    n_lay = np.diff(lay.first_layout.astype(np.int64))
    assert (n_lay == 1).any() and (n_lay == 2).any()
    ret = np.zeros(lay.layouts.size, np.int32)
    sub = SR.host_clique_merge_layouts(e, out_off, g["reads"], off, nodes, g["vertex_read"], g["vertex_fwd"], st, ret).subreads
    assert (sub["index2"] >= 0).any() and (sub["index2"] == -1).any()
    sizes = {len(q) for q in g["cliques"]}
    assert {2, 3, 12, 13, 16, 17, 40, 63, 64, 65} <= sizes
    deg = np.diff(out_off.astype(np.int64))
    assert {63, 64, 65, 200} <= set(deg.tolist())


def test_refusals():
    doc = CM.load_golden()
    e, out_off, reads = CM.golden_graph(doc)
    off, nodes = SR.clique_csr([doc["cliques"][0]["clique"]])
    with pytest.raises(N.HcError) as err:
        SR.host_clique_merge_layouts(e, out_off, reads, off, nodes, doc["vertex_read"], doc["vertex_fwd"], SR.make_settings(min_clique_size=0))
    assert err.value.status == -1 and "min_clique_size" in str(err.value)
    with pytest.raises(N.HcError) as err:
        SR.host_clique_merge_layouts(e, out_off, reads, np.asarray([0, 3, 2], np.uint64), nodes[:2], doc["vertex_read"], doc["vertex_fwd"], SR.make_settings(min_clique_size=2))
    assert err.value.status == -1
    with pytest.raises(N.HcError):
        SR.host_clique_filter([1, 2, 3], [5, 6, 7], 2, 9)  # the base is no entry
    with pytest.raises(N.HcError):
        SR.host_clique_filter([1, 2, 3], [5, 6, 7], 4, 1)  # num exceeds the distinct vertices (assert, :619)
    empty = SR.host_clique_merge_layouts(e, out_off, reads, np.zeros(1, np.uint64), np.zeros(0, np.uint32), doc["vertex_read"], doc["vertex_fwd"],
                                         SR.make_settings(min_clique_size=2))
    assert empty.clique_status.size == 0 and empty.first_layout.tolist() == [0] and empty.layouts.size == 0


def test_group_rule_never_calls_a_tie_dependent_layout_tie_independent():
    """Seeded layouts of 13 - 40 entries, every length: where the rule says HC_SR_FILTER_GROUPS, reversing the order inside the endpos groups
    (and std::sort's own order) selects the same vertices; where it says HC_SR_FILTER_STABLE (at most 16 entries), std::sort's selection is
    the stable order's.  The three classes all occur, and the reversed order does change the selection of some cut layout."""
    rng = np.random.default_rng(17)
    seen, changed = set(), 0
    for n in range(13, 41):
        for rep in range(60):
            n_vertices = int(rng.integers(max(n // 2, 9), n + 1))  # fewer vertices than entries: a paired read in an 's' layout is listed twice
            vertex = np.concatenate([rng.permutation(n_vertices), rng.integers(0, n_vertices, n - n_vertices)]).astype(np.uint32)
            rng.shuffle(vertex)
            endpos = rng.integers(100, 100 + int(rng.choice([3, 6, 40])), n).astype(np.int32)
            num = 2 * int(rng.choice([1, 2, 4]))
            base = int(vertex[rng.integers(0, n)])
            ref, cls = SR.host_clique_filter(vertex, endpos, num, base, 0)
            stable, cls1 = SR.host_clique_filter(vertex, endpos, num, base, 1)
            rev, cls2 = SR.host_clique_filter(vertex, endpos, num, base, 2)
            assert cls == cls1 == cls2 and cls in (SR.SR_FILTER_GROUPS, SR.SR_FILTER_STABLE, SR.SR_FILTER_HOST)
            seen.add(cls)
            assert len(set(vertex[ref.astype(bool)].tolist())) == num
            if cls == SR.SR_FILTER_GROUPS:
                assert np.array_equal(ref, stable) and np.array_equal(ref, rev), (n, rep)
            else:
                assert (cls == SR.SR_FILTER_STABLE) == (n <= 16)
                changed += not np.array_equal(stable, rev)
                if cls == SR.SR_FILTER_STABLE:
                    assert np.array_equal(ref, stable), (n, rep)
    assert seen == {SR.SR_FILTER_GROUPS, SR.SR_FILTER_STABLE, SR.SR_FILTER_HOST} and changed >= 20
