"""hc_sr_merge_next on the device (include/hcsr.h) against the host mirror, every output array for equality: hand-made edge-merge results
over kept bytes loaded with hc_sr_kept_load (no graph needed) at the sizes where a kernel's last workgroup, wave or lane changes; one chain
of 2 000 vertices through hc_graph_load -> hc_graph_merge_pairs -> hc_sr_edge_merge -> the call, whose store must be the one hc_set_reads
loads from the mirror's arrays and whose tables must give find-next-overlaps the mirror's text; the call against hc_sr_set_next_reads on the
equivalent entry list; and the refusals, which leave the old store usable."""
import ctypes as C
import functools

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR
from haploconduct_amd import fno
from haploconduct_amd import host
from haploconduct_amd import merge_next as MN
from haploconduct_amd import next_reads as NR
from tests import _edge_merge as EM
from tests import _merge_next as M
from tests.test_gpu_next_reads import _candidates, _same_readset

pytestmark = pytest.mark.gpu


def _device(c, sc=None, **kw):
    """the call on a fresh context holding c's store and kept bytes -> (result, the new raw arrays or None, store info)"""
    own = sc is None
    sc = sc or hc.EdgeScorer()
    try:
        sc.sr_keep_device(True)
        sc.set_reads(c.reads)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        res = sc.sr_merge_next(c.pairs, c.edge, c.vertex_read, c.vertex_fwd, **kw)
        return res, sc.sr_next_reads_fetch(), sc.info()
    finally:
        if own:
            sc.close()


def _against_mirror(c, kw):
    call, _ = M.split_kw(c, kw)
    ref = M.call_host(c, **call)
    dev, raw, _ = _device(c, **call)
    M.assert_same(dev, ref, str(kw))
    _same_readset(raw, c.reads if ref.empty else ref.reads, "the raw arrays after the call")
    return dev, ref


@pytest.mark.parametrize("nv", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("npairs", [0, 1, 64, 65])
def test_device_equals_the_mirror(nv, npairs):
    """n_pairs beyond n_vertices / 2 makes pairs share vertices; one vertex alone makes the only possible pair (0, 0), which is refused"""
    c = M.make_case(31 * nv + npairs, nv, npairs, reuse_vertex=True)
    for kw in (M.KW_SETS[0], M.KW_SETS[4]):  # nothing set, NULL arrays; every setting, both arrays given
        _against_mirror(c, kw)


def test_every_branch_next_to_every_other():
    """self-merged pairs next to unmerged ones, a dropped super-read whose vertices come back as trivials, reverse paired trivials, a vertex
    named by two pairs, inclusions and tips"""
    c = M.make_case(7, 129, 64, reuse_vertex=True)
    for kw in M.KW_SETS:
        dev, ref = _against_mirror(c, kw)
    call, _ = M.split_kw(c, M.KW_SETS[4])
    dev = _device(c, **call)[0]
    assert set(dev.pair_kind.tolist()) == set(range(6)) and set(dev.vertex_state.tolist()) == set(range(6))
    assert 0 < dev.n_self_merged < (dev.pair_kind >= MN.MN_SINGLE).sum()
    dropped = np.flatnonzero((dev.pair_kind == MN.MN_DROPPED_N_RATE) | (dev.pair_kind == MN.MN_DROPPED_EMPTY))
    back = [v for i in dropped for v in c.pairs[i] if dev.vertex_state[v] == MN.MN_V_TRIVIAL]
    assert back and all(dev.nodes["id"][v] >= dev.n_singles and not dev.nodes["visited"][v] for v in back)
    first = c.reads.read_first_seq.astype(np.int64)
    rev_paired = [v for v in range(129) if dev.vertex_state[v] == MN.MN_V_TRIVIAL and not c.vertex_fwd[v] and first[c.vertex_read[v] + 1] - first[c.vertex_read[v]] == 2]
    assert rev_paired
    counts = np.bincount(c.pairs.reshape(-1), minlength=129)
    assert (counts > 1).any()


def test_all_paired_store_and_a_second_call_on_the_new_store():
    c = M.make_case(11, 65, 30, all_paired=True)
    ref = M.call_host(c)
    with hc.EdgeScorer() as sc:
        dev, raw, _ = _device(c, sc)
        M.assert_same(dev, ref, "all paired")
        _same_readset(raw, ref.reads, "all paired")
        # the next iteration: the new reads as vertices of their own, no pairs — every read comes back as a trivial in order
        n = ref.reads.n_reads
        c2 = M.Case(ref.reads, c.cons_seq, c.cons_qual, np.zeros((0, 2), np.uint32), M.empty_edge(), np.arange(n, dtype=np.uint32), np.ones(n, np.uint8), None, None)
        ref2 = M.call_host(c2)
        dev2 = sc.sr_merge_next(c2.pairs, c2.edge, c2.vertex_read, c2.vertex_fwd)
        M.assert_same(dev2, ref2, "second iteration")
        _same_readset(sc.sr_next_reads_fetch(), ref2.reads, "second iteration")


def test_same_raw_arrays_as_hc_sr_set_next_reads_on_the_equivalent_entry_list():
    c = M.make_case(7, 129, 64)
    kw = dict(keep_singletons=8, ignore_inclusions=True, store_tips_separately=True, inclusions=c.inclusions, tip_reads=c.tip_reads)
    dev, raw, info = _device(c, **kw)
    e, off = c.edge, c.edge.result.out_off.astype(np.int64)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(c.reads)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        # what a caller did before: the self-overlap test on the kept bytes for the paired super-reads with two mates, ...
        cand = [i for i in range(len(c.pairs)) if dev.pair_kind[i] != MN.MN_NONE and e.first_layout[i + 1] - e.first_layout[i] == 2 and
                all(e.result.status[int(e.first_layout[i]) + k] == 0 and off[int(e.first_layout[i]) + k + 1] > off[int(e.first_layout[i]) + k] for k in (0, 1))]
        sp = np.array([(off[int(e.first_layout[i])], off[int(e.first_layout[i]) + 1], off[int(e.first_layout[i]) + 1] - off[int(e.first_layout[i])],
                        off[int(e.first_layout[i]) + 2] - off[int(e.first_layout[i]) + 1]) for i in cand], SR.SR_PAIR_DTYPE)
        m = sc.sr_merge_self_overlaps_kept(sp)
        merged = {i: (int(m.out_off[k]), int(m.out_off[k + 1] - m.out_off[k])) for k, i in enumerate(cand) if m.status[k] == SR.SR_SELF_MERGED}
        assert sorted(merged) == np.flatnonzero(dev.pair_kind == MN.MN_SINGLE_SELF).tolist()
        # ... and the entry list by hand: singles, trivials, pairs — only what the new call says survives or is a trivial
        singles, pairs_ = [], []
        for i in range(len(c.pairs)):
            l0 = int(e.first_layout[i])
            if dev.pair_kind[i] == MN.MN_SINGLE_SELF:
                singles.append(NR.single(*merged[i]))
            elif dev.pair_kind[i] == MN.MN_SINGLE:
                singles.append(NR.single(off[l0], off[l0 + 1] - off[l0]))
            elif dev.pair_kind[i] == MN.MN_PAIRED:
                pairs_.append(NR.paired(off[l0], off[l0 + 1] - off[l0], off[l0 + 1], off[l0 + 2] - off[l0 + 1]))
        trivials = [NR.trivial(int(c.vertex_read[v]), not c.vertex_fwd[v], c.reads.is_paired(int(c.vertex_read[v])))
                    for v in np.flatnonzero(dev.vertex_state == MN.MN_V_TRIVIAL)]
        res = sc.sr_set_next_reads(np.array(singles + trivials + pairs_, NR.NEXT_ENTRY_DTYPE), keep_singletons=8)
        assert (res.status == NR.NEXT_KEPT).all() and res.new_id.tolist() == list(range(dev.new_read_count))
        _same_readset(sc.sr_next_reads_fetch(), raw, "hc_sr_set_next_reads on the equivalent entry list")
        assert sc.info() == info


@functools.lru_cache(maxsize=None)
def _chain():
    g = EM.seeded_graph()
    g["csr"] = EM.csr(g["V"], g["rows"])
    return g


def test_a_chain_of_2000_vertices_store_and_find_next_overlaps():
    g = _chain()
    kw = dict(keep_singletons=100)
    with hc.EdgeScorer() as sc, hc.EdgeScorer() as sc2:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.graph_load(*g["csr"])
        pairs = sc.graph_merge_pairs()
        assert pairs.shape[0] > 400
        edge = sc.sr_edge_merge(pairs, g["vertex_read"], g["vertex_fwd"])
        ref = host.sr_merge_next(g["reads"], edge.result.cons_seq, edge.result.cons_qual, pairs, edge, g["vertex_read"], g["vertex_fwd"], **kw)
        dev = sc.sr_merge_next(pairs, edge, g["vertex_read"], g["vertex_fwd"], **kw)
        M.assert_same(dev, ref, "chain")
        assert dev.n_self_merged > 50 and dev.n_trivials > 500 and dev.counts["n_dropped_short"] > 20 and dev.ms_device > 0
        _same_readset(sc.sr_next_reads_fetch(), ref.reads, "chain")
        # the store is the one hc_set_reads loads from the mirror's arrays
        sc2.set_reads(ref.reads)
        assert sc.info() == sc2.info() and sc.kernel_info() == sc2.kernel_info()
        cand = hc.EdgeScorer.pack_cands(_candidates(np.random.default_rng(3), ref.reads, 2000))
        assert sc.score_cands(cand).tobytes() == sc2.score_cands(cand).tobytes()
        # find-next-overlaps fed from the returned tables as they are
        ge = fno.edges_from_graph(sc.graph_fetch()["edges"])
        text_dev, counters_dev = fno.find_next_overlaps(dev.fno1_input(ge))
        text_ref, counters_ref = fno.find_next_overlaps(ref.fno1_input(ge))
        assert text_dev == text_ref and counters_dev == counters_ref and counters_dev["n_lines"] > 100


def test_refusals_leave_the_old_store_usable():
    c = M.make_case(3, 20, 6)
    with hc.EdgeScorer() as sc:
        with pytest.raises(hc.HcError, match="hc_sr_keep_device is off") as e:
            sc.sr_merge_next(c.pairs, c.edge, c.vertex_read, c.vertex_fwd)
        assert e.value.status == -5  # HC_ERR_STATE
        sc.sr_keep_device(True)
        with pytest.raises(hc.HcError, match="no store whose raw arrays were kept"):
            sc.sr_merge_next(c.pairs, c.edge, c.vertex_read, c.vertex_fwd)
        sc.set_reads(c.reads)
        with pytest.raises(hc.HcError, match="no kept consensus bytes"):
            sc.sr_merge_next(c.pairs, c.edge, c.vertex_read, c.vertex_fwd)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        # HC_ERR_ARG: n_pairs + n_vertices >= 2^31 is refused before anything is read
        inp, st, out = MN.hc_sr_merge_next_input(), MN.hc_sr_merge_next_settings(), MN.hc_sr_merge_next_output()
        inp.n_pairs, inp.n_vertices = 1 << 30, 1 << 30
        assert N.lib.hc_sr_merge_next(sc._ctx, C.byref(inp), C.byref(st), C.byref(out)) == -1
        bad = SR.SrEdgeLayouts(c.edge.pair_status, c.edge.first_layout + np.uint64(100), c.edge.layouts, c.edge.members, c.edge.subreads, c.edge.result)
        with pytest.raises((hc.HcError, ValueError)):
            sc.sr_merge_next(c.pairs, bad, c.vertex_read, c.vertex_fwd)
        _same_readset(sc.sr_next_reads_fetch(), c.reads, "the old store stays")
        # an empty result keeps it too
        c0 = M.Case(c.reads, c.cons_seq, c.cons_qual, np.zeros((0, 2), np.uint32), M.empty_edge(), c.vertex_read, c.vertex_fwd, None, None)
        empty = sc.sr_merge_next(c0.pairs, c0.edge, c0.vertex_read, c0.vertex_fwd, keep_singletons=10 ** 6)
        assert empty.empty and (empty.vertex_state == MN.MN_V_SHORT).all()
        M.assert_same(empty, M.call_host(c0, keep_singletons=10 ** 6), "nothing survives")
        _same_readset(sc.sr_next_reads_fetch(), c.reads, "the old store stays")
        # and the call still works afterwards
        dev = sc.sr_merge_next(c.pairs, c.edge, c.vertex_read, c.vertex_fwd)
        M.assert_same(dev, M.call_host(c), "after the refusals")
