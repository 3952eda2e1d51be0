"""hc_sr_clique_next on the device (include/hcsr.h) against the host mirror, every output array and the fetched raw store for equality:
hand-made clique-merge results over kept bytes loaded with hc_sr_kept_load (no graph needed) at the sizes where a kernel's last workgroup,
wave or lane changes; one real chain hc_graph_load -> hc_sr_clique_merge -> the call, whose store must be the one hc_set_reads loads from
the mirror's arrays and whose tables must give find-next-overlaps the mirror's text; two-vertex cliques against hc_sr_merge_next on one
context; a second call on the new store; and the refusals, which leave the old store usable."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import clique_next as CN
from haploconduct_amd import consensus as SR
from haploconduct_amd import fno
from haploconduct_amd import host
from haploconduct_amd import merge_next as MN
from tests import _clique_merge as CM
from tests import _clique_next as Q
from tests import _edge_merge as EM
from tests.test_gpu_next_reads import _same_readset

pytestmark = pytest.mark.gpu

# n_vertices, clique sizes (n_cliques in {0, 1, 64, 65}; sizes 2, 3, 16, 17, 63, 64, 65, 200; the items cross 256 and 512), overlapping
CASES = [
    (1, [], False),
    (1, [1], False),                                            # one vertex alone: its clique is refused
    (63, [3], False),
    (63, [2, 3] * 32, True),                                    # 64 cliques, 160 items
    (64, [2, 3, 16, 17] * 16 + [5], True),                      # 65 cliques, 613 items
    (65, [63], False),
    (65, [4] * 64, True),                                       # 256 items
    (65, [4] * 63 + [5, 2], True),                              # 259 items
    (257, [64, 65, 63, 17, 16, 3, 2], False),
    (257, [200, 17, 2], False),
    (257, [8] * 64 + [3], True),                                # 515 items
]


def _case(k):
    nv, sizes, overlap = CASES[k]
    return Q.make_case(4000 + k, nv, sizes, overlap=overlap)


def _device(c, sc=None, **kw):
    """the call on a fresh context holding c's store and kept bytes -> (result, the new raw arrays, store info)"""
    own = sc is None
    sc = sc or hc.EdgeScorer()
    try:
        sc.sr_keep_device(True)
        sc.set_reads(c.reads)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        res = sc.sr_clique_next(c.clique_off, c.clique_nodes, c.merged, c.vertex_read, c.vertex_fwd, **kw)
        return res, sc.sr_next_reads_fetch(), sc.info()
    finally:
        if own:
            sc.close()


def _against_mirror(c, kw):
    ref = Q.call_host(c, **kw)
    dev, raw, _ = _device(c, **kw)
    Q.assert_same(dev, ref, str(kw))
    _same_readset(raw, c.reads if ref.empty else ref.reads, "the raw arrays after the call")
    return dev, ref


@pytest.mark.parametrize("k", range(len(CASES)))
def test_device_equals_the_mirror(k):
    c = _case(k)
    for kw in (Q.KW_SETS[0], Q.KW_SETS[1]):
        _against_mirror(c, kw)


def test_the_cases_hold_every_branch():
    """every kind, the vertex states, a dropped clique whose vertices return as trivials, overlapping cliques, a filtered layout whose unused
    members still get marked, a reverse paired trivial, unsorted input cliques — computed by the mirror, which the device equals above"""
    kinds, states = set(), set()
    back = overlapping = unused_marked = rev_paired = unsorted = 0
    for k in range(len(CASES)):
        c = _case(k)
        got = Q.call_host(c, keep_singletons=8)
        kinds |= set(got.clique_kind.tolist())
        states |= set(got.vertex_state.tolist())
        n = len(c.clique_off) - 1
        dropped = np.flatnonzero((got.clique_kind == MN.MN_DROPPED_N_RATE) | (got.clique_kind == MN.MN_DROPPED_EMPTY))
        back += sum(got.vertex_state[v] == MN.MN_V_TRIVIAL and not got.nodes["visited"][v] for i in dropped for v in Q.clique(c, i))
        overlapping += (np.bincount(c.clique_nodes, minlength=1) > 1).any()
        for i in np.flatnonzero(got.clique_kind >= MN.MN_SINGLE):
            L = c.merged.layouts[int(c.merged.first_layout[i])]
            a = int(L["first_member"])
            for m in range(a, a + int(L["n_members"])):
                if not c.merged.member_used[m]:
                    assert got.vertex_state[c.merged.member_vertex[m]] == MN.MN_V_MERGED
                    unused_marked += 1
        first = c.reads.read_first_seq.astype(np.int64)
        rev_paired += sum(got.vertex_state[v] == MN.MN_V_TRIVIAL and not c.vertex_fwd[v] and first[c.vertex_read[v] + 1] - first[c.vertex_read[v]] == 2
                          for v in range(len(c.vertex_read)))
        unsorted += any(Q.clique(c, i) != sorted(Q.clique(c, i)) for i in range(n))
    assert kinds == set(range(6))
    assert states >= {MN.MN_V_MERGED, MN.MN_V_TRIVIAL, MN.MN_V_SHORT, MN.MN_V_N_RATE}  # (MN_V_BAD: the test below)
    assert back and overlapping and unused_marked and rev_paired and unsorted


def test_a_vertex_whose_read_is_not_in_the_store():
    c = _case(2)
    c.vertex_read = c.vertex_read.copy()
    free = [v for v in range(len(c.vertex_read)) if v not in set(c.clique_nodes.tolist())]
    c.vertex_read[free[0]] = c.reads.n_reads + 5
    dev, ref = _against_mirror(c, {})
    assert dev.vertex_state[free[0]] == MN.MN_V_BAD and dev.nodes["visited"][free[0]] == 1 and dev.counts["n_bad"] >= 1


def test_a_self_merged_clique_of_more_than_64_entries_with_ties():
    c = Q.make_case(77, 120, [40, 33, 2, 41], all_paired=True, force=0.5)
    dev, ref = _against_mirror(c, {})
    assert dev.n_self_merged == 4 and [len(dev.row(k)) for k in range(4)] == [80, 66, 4, 82]
    want, store = Q.restatement(c)
    Q.check_against_restatement(dev, want, store)
    sub = dev.subreads[int(dev.subread_off[0]):int(dev.subread_off[1])]
    idx = sub["index1"].tolist() + sub["index2"].tolist()
    assert len(set(idx)) < len(idx) / 4  # many equal indexes: the row's order is the documented tie order, which the restatement states


@pytest.mark.parametrize("seed,nv,n", [(2, 64, 32), (3, 131, 65)])
def test_two_vertex_cliques_equal_hc_sr_merge_next_on_one_context(seed, nv, n):
    c = Q.make_case(seed, nv, [2] * n, overlap=2 * n > nv)
    p = Q.as_pairs_case(c)
    with hc.EdgeScorer() as sc:
        a, raw_a, info_a = _device(c, sc, keep_singletons=8)
        sc.set_reads(c.reads)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        b = sc.sr_merge_next(p.pairs, p.edge, p.vertex_read, p.vertex_fwd, keep_singletons=8)
        raw_b, info_b = sc.sr_next_reads_fetch(), sc.info()
    for ka, kb in (("clique_kind", "pair_kind"), ("clique_new_id", "pair_new_id"), ("sr_clique", "sr_pair")):
        assert np.array_equal(getattr(a, ka), getattr(b, kb)), ka
    for k in ("overlap_pos", "self_score", "vertex_state", "nodes", "srs", "clique_off", "clique_nodes", "subread_off", "subreads"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    for k in ("n_singles", "n_trivials", "n_paired", "n_self_merged", "new_read_count", "empty"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("n_kept", "n_dropped_empty", "n_dropped_n_rate", "n_dropped_short", "n_bad", "n_seq", "n_bytes"):
        assert a.counts[k] == b.counts[k], k
    _same_readset(raw_a, raw_b, "the stores of the two calls")
    assert info_a == info_b and a.n_self_merged > 0


def test_a_second_call_on_the_new_store():
    c = Q.make_case(11, 65, [3, 4, 5, 6, 7, 8], all_paired=True)
    ref = Q.call_host(c)
    with hc.EdgeScorer() as sc:
        dev, raw, _ = _device(c, sc)
        Q.assert_same(dev, ref, "all paired")
        _same_readset(raw, ref.reads, "all paired")
        # the next iteration: the new reads as vertices of their own, no cliques — every read comes back as a trivial in order
        n = ref.reads.n_reads
        e = np.zeros(0, np.uint8)
        none = Q.merged_of([], [0], np.zeros(0, SR.SR_LAYOUT_DTYPE), [], [], np.zeros(0, SR.SR_SUBREAD_DTYPE), [], [0], e, e)
        c2 = Q.Case(ref.reads, c.cons_seq, c.cons_qual, np.zeros(1, np.uint64), np.zeros(0, np.uint32), none, np.arange(n, dtype=np.uint32), np.ones(n, np.uint8))
        ref2 = Q.call_host(c2)
        dev2 = sc.sr_clique_next(c2.clique_off, c2.clique_nodes, c2.merged, c2.vertex_read, c2.vertex_fwd)
        Q.assert_same(dev2, ref2, "second iteration")
        assert dev2.n_trivials == n
        _same_readset(sc.sr_next_reads_fetch(), ref2.reads, "second iteration")


@functools.lru_cache(maxsize=None)
def _chain():
    g = CM.seeded_cliques()
    g["csr"] = EM.csr(g["V"], g["rows"])
    g["off"], g["nodes"] = SR.clique_csr(g["cliques"])
    return g


def test_a_real_chain_store_and_find_next_overlaps():
    g = _chain()
    kw = dict(keep_singletons=50)
    with hc.EdgeScorer() as sc, hc.EdgeScorer() as sc2:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.graph_load(*g["csr"])
        merged = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        ref = host.sr_clique_next(g["reads"], merged.result.cons_seq, merged.result.cons_qual, g["off"], g["nodes"], merged, g["vertex_read"],
                                  g["vertex_fwd"], **kw)
        dev = sc.sr_clique_next(g["off"], g["nodes"], merged, g["vertex_read"], g["vertex_fwd"], **kw)
        Q.assert_same(dev, ref, "chain")
        assert len(dev.srs) > 50 and dev.ms_device > 0 and not dev.empty
        _same_readset(sc.sr_next_reads_fetch(), ref.reads, "chain")
        # the store is the one hc_set_reads loads from the mirror's arrays
        sc2.set_reads(ref.reads)
        assert sc.info() == sc2.info() and sc.kernel_info() == sc2.kernel_info()
        # find-next-overlaps fed from the returned tables as they are
        ge = fno.edges_from_graph(sc.graph_fetch()["edges"])
        text_dev, counters_dev = fno.find_next_overlaps(dev.fno1_input(ge))
        text_ref, counters_ref = fno.find_next_overlaps(ref.fno1_input(ge))
        assert text_dev == text_ref and counters_dev == counters_ref


def test_refusals_leave_the_old_store_usable():
    c = Q.make_case(3, 30, [3, 4, 5])
    args = (c.clique_off, c.clique_nodes, c.merged, c.vertex_read, c.vertex_fwd)
    with hc.EdgeScorer() as sc:
        with pytest.raises(hc.HcError, match="hc_sr_keep_device is off") as e:
            sc.sr_clique_next(*args)
        assert e.value.status == -5  # HC_ERR_STATE
        sc.sr_keep_device(True)
        with pytest.raises(hc.HcError, match="no store whose raw arrays were kept"):
            sc.sr_clique_next(*args)
        sc.set_reads(c.reads)
        with pytest.raises(hc.HcError, match="no kept consensus bytes"):
            sc.sr_clique_next(*args)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        # HC_ERR_ARG: n_cliques + n_vertices >= 2^31 is refused before anything is read
        inp, st, out = CN.hc_sr_clique_next_input(), CN.hc_sr_clique_next_settings(), CN.hc_sr_clique_next_output()
        inp.n_cliques, inp.n_vertices = 1 << 30, 1 << 30
        assert N.lib.hc_sr_clique_next(sc._ctx, C.byref(inp), C.byref(st), C.byref(out)) == -1
        with pytest.raises(hc.HcError, match="clique_off descends"):
            sc.sr_clique_next(np.array([0, 7, 3, 12], np.uint64), *args[1:])
        _same_readset(sc.sr_next_reads_fetch(), c.reads, "the old store stays")
        # a clique with a vertex outside the graph is refused alone, the others go on
        nodes = c.clique_nodes.copy()
        nodes[4] = 30
        ref = host.sr_clique_next(c.reads, c.cons_seq, c.cons_qual, c.clique_off, nodes, *args[2:])
            # an empty result keeps the store: no clique owns a super-read and every vertex is too short
        none = copy.copy(c.merged)
        none.clique_status = np.full(3, 3, np.uint32)
        got = sc.sr_clique_next(c.clique_off, nodes, none, *args[3:], keep_singletons=10 ** 6)
        assert got.empty and (got.vertex_state == MN.MN_V_SHORT).all() and not got.clique_kind.any()
        Q.assert_same(got, host.sr_clique_next(c.reads, c.cons_seq, c.cons_qual, c.clique_off, nodes, none, *args[3:], keep_singletons=10 ** 6), "nothing survives")
        _same_readset(sc.sr_next_reads_fetch(), c.reads, "the old store stays")
        # and the call still works afterwards
        dev = sc.sr_clique_next(c.clique_off, nodes, *args[2:])
        Q.assert_same(dev, ref, "after the refusals")
        assert dev.clique_kind[1] == MN.MN_NONE and not dev.empty
        _same_readset(sc.sr_next_reads_fetch(), ref.reads, "after the refusals")
