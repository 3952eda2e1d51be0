"""The clique merge on the device graph (include/hcsr.h: hc_sr_clique_merge) against the reference's own constructSuperread
(tests/golden/clique_merge.json), against the host mirror on a seeded graph of cliques array by array, against hc_sr_consensus fed the
mirror's USED members from the host (8-bit and 16-bit store, error correction), the kept bytes behind hc_sr_set_next_reads, every filtered
layout decided on the host, cliques of two against hc_sr_edge_merge, and the call-level statuses.  (The preconditions on the seeded graph are
asserted on the mirror's output: tests/test_clique_merge_host.py.)"""
import functools

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import consensus as SR
from haploconduct_amd import host
from haploconduct_amd import next_reads as NR
from tests import _clique_merge as CM
from tests import _edge_merge as EM
from tests import _sr

pytestmark = pytest.mark.gpu

DOC = CM.load_golden()
GROUPS = sorted(CM.golden_groups(DOC).items())


@functools.lru_cache(maxsize=None)
def seeded(quals=(50, 74), error_correction=False):
    """The seeded cliques, the graph's CSR form, the mirror's layouts, the mirror's consensus of the USED members and the mirror's subread
    infos for its return values — computed once, left unchanged."""
    g = CM.seeded_cliques(quals=quals)
    g["csr"] = EM.csr(g["V"], g["rows"])
    g["off"], g["nodes"] = SR.clique_csr(g["cliques"])
    st = SR.make_settings(min_clique_size=g["m"], error_correction=error_correction)
    args = (g["csr"][0], g["csr"][1], g["reads"], g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], st)
    m = SR.host_clique_merge_layouts(*args)
    g["used"] = m.used_layouts()
    g["cons"] = host.sr_consensus(g["reads"], *g["used"], min_clique_size=g["m"], error_correction=error_correction, n_threads=16)
    g["mirror"] = SR.host_clique_merge_layouts(*args, ret=g["cons"].ret)
    assert np.array_equal(m.clique_status, g["want_status"])
    return g


def load(sc, g):
    sc.set_reads(g["reads"])
    sc.graph_load(*g["csr"])


@pytest.mark.parametrize("key,cliques", GROUPS, ids=[f"m{m}-ec{ec}" for (m, ec), _ in GROUPS])
def test_device_equals_the_reference_on_every_golden_clique(key, cliques):
    m, ec = key
    want = CM.golden_arrays(cliques)
    e, out_off, reads = CM.golden_graph(DOC)
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        sc.graph_load(*EM.csr(DOC["V"], DOC["edges_in"]))
        got = sc.sr_clique_merge(want[0], want[1], DOC["vertex_read"], DOC["vertex_fwd"], min_clique_size=m, error_correction=bool(ec))
    # (the trim positions depend on positions and lengths alone, so the device's own consensus returns the reference's)
    assert np.array_equal(got.result.ret, want[7]), "trim positions differ"
    CM.assert_equal_layouts(got, want, f"m={m} ec={ec}")


def test_device_equals_the_mirror_on_seeded_cliques():
    g = seeded()
    with hc.EdgeScorer() as sc:
        load(sc, g)
        got = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
    m = g["mirror"]
    assert np.array_equal(got.clique_status, g["want_status"])
    assert np.array_equal(got.result.ret, g["cons"].ret)
    CM.assert_equal_layouts(got, m, "seeded cliques")
    assert got.n_filtered_layouts == m.n_filtered_layouts >= 40 and got.n_host_filters == m.n_host_filters >= 10
    assert got.ms_layout > 0 and got.ms_host_filter > 0


@pytest.mark.parametrize("quals", [(50, 74), (33, 104)], ids=["8-bit store", "16-bit store"])
def test_consensus_bytes_equal_hc_sr_consensus_fed_the_used_members(quals):
    g = seeded(quals)
    with hc.EdgeScorer() as sc:
        load(sc, g)
        assert sc.info()["qual_alphabet"] == quals[1] - quals[0]
        got = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        fed = sc.sr_consensus(*g["used"], min_clique_size=g["m"])
    _sr.assert_same(got.result, fed, "clique merge against hc_sr_consensus")
    _sr.assert_same(got.result, g["cons"], "clique merge against the mirror's consensus")
    assert (np.diff(fed.out_off.astype(np.int64)) > 0).mean() >= 0.9


def test_error_correction():
    g = seeded(error_correction=True)
    with hc.EdgeScorer() as sc:
        load(sc, g)
        got = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"], error_correction=True)
        fed = sc.sr_consensus(*g["used"], min_clique_size=g["m"], error_correction=True)
    _sr.assert_same(got.result, fed, "error correction")
    CM.assert_equal_layouts(got, g["mirror"], "error correction")
    assert (got.result.ret > 0).any() and (got.result.ret == -1).any() and (got.subreads["startpos1"] > 0).any()


def test_next_store_after_clique_merge_equals_the_one_after_hc_sr_consensus():
    g = seeded()
    m, cons = g["mirror"], g["cons"]
    off = cons.out_off.astype(np.int64)
    entries = []
    for i in range(len(g["cliques"])):
        l0, l1 = int(m.first_layout[i]), int(m.first_layout[i + 1])
        if l1 - l0 == 2:
            entries.append(NR.paired(off[l0], off[l0 + 1] - off[l0], off[l0 + 1], off[l0 + 2] - off[l0 + 1]))
        elif l1 - l0 == 1:
            entries.append(NR.single(off[l0], off[l0 + 1] - off[l0]))
    entries = np.array(entries + [NR.trivial(0, is_paired=g["reads"].is_paired(0))], NR.NEXT_ENTRY_DTYPE)
    stores = []
    for route in ("clique_merge", "consensus"):
        with hc.EdgeScorer() as sc:
            sc.sr_keep_device(True)
            load(sc, g)
            if route == "clique_merge":
                sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
            else:
                sc.sr_consensus(*g["used"], min_clique_size=g["m"])
            res = sc.sr_set_next_reads(entries)
            assert not res.empty
            stores.append((res.status, res.new_id, sc.info(), sc.sr_next_reads_fetch()))
    a, b = stores
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    for k in ("read_first_seq", "seq_off", "bases", "quals"):
        assert np.array_equal(getattr(a[3], k), getattr(b[3], k)), k
    assert (a[0] == NR.NEXT_KEPT).sum() > 100


def test_every_filter_on_the_host_gives_identical_outputs():
    g = seeded()
    with hc.EdgeScorer() as sc:
        load(sc, g)
        a = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        sc.sr_clique_filter_on_host(True)
        b = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        sc.sr_clique_filter_on_host(False)
    CM.assert_equal_layouts(b, a, "every filter on the host")
    _sr.assert_same(b.result, a.result, "every filter on the host")
    assert a.n_filtered_layouts == b.n_filtered_layouts and a.n_host_filters == b.n_host_filters


def test_a_list_of_pairs_gives_exactly_hc_sr_edge_merge():
    g = EM.seeded_graph()
    off, nodes = SR.clique_csr(g["pairs"].tolist())
    case, pairs, want = EM.planted()
    with hc.EdgeScorer() as sc:
        sc.set_reads(g["reads"])
        sc.graph_load(*EM.csr(g["V"], g["rows"]))
        a = sc.sr_edge_merge(g["pairs"], g["vertex_read"], g["vertex_fwd"])
        b = sc.sr_clique_merge(off, nodes, g["vertex_read"], g["vertex_fwd"])
        sc.set_reads(EM.random_reads(case["reads"], 3))
        sc.graph_load(*EM.csr(case["V"], case["edges_in"]))
        pa = sc.sr_edge_merge(pairs, case["vertex_read"], case["vertex_fwd"])
        pb = sc.sr_clique_merge(*SR.clique_csr(pairs), case["vertex_read"], case["vertex_fwd"])
    for x, y in ((a, b), (pa, pb)):
        assert np.array_equal(x.pair_status, y.clique_status)
        assert np.array_equal(x.first_layout, y.first_layout) and np.array_equal(x.layouts, y.layouts) and np.array_equal(x.members, y.members)
        assert np.array_equal(x.subreads.reshape(-1), y.subreads)
        _sr.assert_same(x.result, y.result, "pairs")
        assert y.member_used.all() and (y.layout_filter == SR.SR_FILTER_NONE).all()
    assert pa.pair_status.tolist() == want and (a.pair_status == SR.SR_EDGE_OK).all()


def test_call_level_statuses():
    g = seeded()
    with hc.EdgeScorer() as sc:
        with pytest.raises(hc.HcError, match="hc_set_reads first"):
            sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"])
        sc.set_reads(g["reads"])
        with pytest.raises(hc.HcError, match="no graph"):
            sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"])
        sc.graph_load(*g["csr"])
        with pytest.raises(hc.HcError, match="min_clique_size == 0"):
            sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=0)
        with pytest.raises(hc.HcError, match="n_vertices"):
            sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"][:3], g["vertex_fwd"][:3])
        empty = sc.sr_clique_merge(np.zeros(1, np.uint64), np.zeros(0, np.uint32), g["vertex_read"], g["vertex_fwd"])
        assert empty.clique_status.size == 0 and empty.first_layout.tolist() == [0] and empty.result.out_off.tolist() == [0]
        only_empty = sc.sr_clique_merge(np.zeros(3, np.uint64), np.zeros(0, np.uint32), g["vertex_read"], g["vertex_fwd"])
        assert only_empty.clique_status.tolist() == [SR.SR_CLIQUE_TOO_SMALL] * 2 and only_empty.layouts.size == 0
