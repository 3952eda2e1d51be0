"""hc_sr_originals_init / _load / _fetch / _next / _write_text on the device (include/hcsr.h) against the host mirrors — offsets, entries,
statuses and text bytes for equality: hand-made dicts and tables (no graph needed) at the sizes where a kernel's last workgroup, wave,
lane or bisection step changes; init against the first iteration's dict of a mixed store; one real chain per merge call on one context
(hc_graph_load -> hc_sr_clique_merge -> hc_sr_clique_next -> the call, and hc_sr_edge_merge -> hc_sr_merge_next -> the call) followed by a
second iteration on the new dict with first_it off; and the refusals, which leave the kept dict as it was."""
import functools

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import consensus as SR
from haploconduct_amd import host
from haploconduct_amd import merge_next as MN
from haploconduct_amd import originals as OR
from haploconduct_amd.consensus import SR_LAYOUT_DTYPE
from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE
from haploconduct_amd.readstore import ReadSet
from tests import _clique_merge as CM
from tests import _edge_merge as EM
from tests import _originals as O

pytestmark = pytest.mark.gpu

# n_vertices, super-read sizes, keywords of _originals.make_case.  Sources = the super-reads' vertices + n_vertices: 1, 64, 65 and more;
# dict lists of 1, 63, 64, 65 and 200; candidate totals 252 / 256 / 260 and 504 / 512 / 520; runs as long as the clique; reads without entries
CASES = [
    (1, [], dict(short=0.0)),
    (64, [], dict(short=0.0)),
    (65, [], dict(short=0.0)),
    (63, [], dict(short=0.0, dict_sizes=(4,))),
    (64, [], dict(short=0.0, dict_sizes=(4,))),
    (65, [], dict(short=0.0, dict_sizes=(4,))),
    (63, [], dict(short=0.0, dict_sizes=(8,))),
    (64, [], dict(short=0.0, dict_sizes=(8,))),
    (65, [], dict(short=0.0, dict_sizes=(8,))),
    (30, [2, 3] * 4, dict(first_it=True, dict_sizes=(1,))),
    (60, [2, 3, 5, 8, 2, 3], dict(n_orig=20)),
    (40, [3, 2, 5, 2], dict(dict_sizes=(1, 63, 64, 65, 200), n_orig=1000)),
    (90, [40, 3, 2], dict(dict_sizes=(1, 2, 65), n_orig=400)),
    (60, [40], dict(share=True, dict_sizes=(30,))),
    (257, [64, 65, 63, 17, 16, 3, 2], dict(n_orig=300)),
    (70, [2] * 14, dict(seq0=True)),
    (70, [4] * 9, dict(seq0=True, first_it=True)),
    (50, [3] * 6, dict(wide=True)),
    (50, [3] * 6, dict(empty=0.3)),
    (50, [2] * 10, dict(empty=0.7)),                            # super-reads none of whose members names an original: OK and empty
]


def _dummy_reads(n):
    return ReadSet.from_lists([("ACGTACGTAC", "IIIIIIIIII")] * n, [])


def _case(k):
    nv, sizes, kw = CASES[k]
    return O.make_case(7000 + k, nv, sizes, **kw)


def _n_cand(maps, t):
    n = sum(len(maps[int(t.vertex_read[int(r["node"])])]) for r in t.subreads)
    return n + sum(len(maps[int(t.vertex_read[v])]) for v in np.flatnonzero(t.vertex_state == MN.MN_V_TRIVIAL))


def _same(dev, dict_dev, text_dev, ref, what):
    assert dev.off.tolist() == ref.off.tolist(), what + ": offsets"
    assert dev.status.tolist() == ref.status.tolist(), what + ": statuses"
    assert (dev.n_entries, dev.n_failed) == (ref.n_entries, ref.n_failed), what
    assert dict_dev[0].tolist() == ref.off.tolist() and dict_dev[1].tobytes() == ref.entries.tobytes(), what + ": the kept dict"
    assert text_dev == host.sr_originals_text(ref.off, ref.entries), what + ": text"


def _device(maps, t):
    off, entries = O.to_csr(maps)
    with hc.EdgeScorer() as sc:
        sc.set_reads(_dummy_reads(len(maps)))
        sc.sr_originals_load(off, entries)
        back = sc.sr_originals_fetch()
        assert back[0].tolist() == off.tolist() and back[1].tobytes() == entries.tobytes()
        res = sc.sr_originals_next(t, None, None, None)
        return res, sc.sr_originals_fetch(), sc.sr_originals_text()


@pytest.mark.parametrize("k", range(len(CASES)))
def test_device_equals_the_mirror(k):
    maps, t = _case(k)
    ref = host.sr_originals_next(*O.to_csr(maps), t)
    dev, kept, text = _device(maps, t)
    _same(dev, kept, text, ref, f"case {k}")
    want, status = O.next_restatement(maps, t)
    assert dev.status.tolist() == status.tolist() and text == O.text_restatement(want)
    assert dev.ms_device > 0


def test_the_cases_hold_the_sizes_and_every_status():
    totals, sources, lists, statuses, run, no_entries = set(), set(), set(), set(), 0, 0
    for k in range(len(CASES)):
        maps, t = _case(k)
        totals.add(_n_cand(maps, t))
        sources.add(len(t.subreads) + len(t.vertex_read))
        lists |= set(len(m) for m in maps)
        ref = host.sr_originals_next(*O.to_csr(maps), t)
        statuses |= set(ref.status.tolist())
        no_entries += int(((np.diff(ref.off.astype(np.int64)) == 0) & (ref.status == 0)).sum())
        for j in range(len(t.sr_clique)):
            rows = t.subreads[int(t.subread_off[j]):int(t.subread_off[j + 1])]
            ids = [tuple(sorted(maps[int(t.vertex_read[int(r["node"])])])) for r in rows]
            if len(rows) == 40 and len(set(ids)) == 1 and len(ids[0]) == 30:
                run += 1
    assert totals >= {252, 256, 260, 504, 512, 520} and max(totals) > 2000
    assert sources >= {1, 64, 65} and lists >= {1, 63, 64, 65, 200}
    assert statuses == {0, 1, 2, 3} and run == 1 and no_entries > 0


def test_no_sources_at_all():
    e = np.zeros(0, np.uint32)
    t = OR.Tables(e, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, SR_LAYOUT_DTYPE), e, np.zeros(1, np.uint64),
                  np.zeros(0, FNO_SUBREAD_DTYPE), e, np.zeros(0, FNO_READ_DTYPE), e, np.zeros(0, np.uint8), 0, False)
    maps = [{0: dict(index1=1, index2=0, len1=10, len2=0, paired=False, forward=True)}]
    dev, kept, text = _device(maps, t)
    assert dev.off.tolist() == [0] and dev.n_entries == 0 and kept[0].tolist() == [0] and kept[1].size == 0 and text == b""


def test_text_digits_and_signs():
    """original ids and indices of 1, 2, 9 and 10 digits, negative ones, line ids crossing 9 -> 10"""
    values = [0, 5, 42, 123456789, 2147483647, -1, -42, -123456789, -2147483648]
    ids = [0, 9, 10, 99, 123456789, 4294967295]
    maps = []
    for r in range(12):
        m = {}
        for j, oid in enumerate(ids[:1 + r % len(ids)]):
            p = (r + j) % 2 == 0
            m[oid] = dict(index1=values[(r + j) % len(values)], index2=values[(r + 2 * j + 3) % len(values)] if p else 0, len1=[7, 150, 1000000000][j % 3],
                          len2=[9, 99, 250][j % 3] if p else 0, paired=p, forward=(r + j) % 3 == 0)
        maps.append(m)
    maps[5] = {}
    off, entries = O.to_csr(maps)
    with hc.EdgeScorer() as sc:
        sc.set_reads(_dummy_reads(len(maps)))
        sc.sr_originals_load(off, entries)
        text = sc.sr_originals_text()
        # a range of it
        from haploconduct_amd import _native as N

        part = np.zeros(11, np.uint8)
        N.check(N.lib.hc_sr_originals_text_fetch(sc._ctx, 3, 11, part.ctypes.data), "hc_sr_originals_text_fetch")
        assert N.lib.hc_sr_originals_text_fetch(sc._ctx, len(text) - 3, 4, part.ctypes.data) == -1
    assert text == host.sr_originals_text(off, entries) == O.text_restatement(maps)
    assert part.tobytes() == text[3:14] and b"\n5\n" in text and b":-2147483648" in text and b"\t4294967295:" in text
    back = host.sr_originals_parse(text)
    assert back[0].tolist() == off.tolist() and back[1].tobytes() == entries.tobytes()


def _first_dict(reads):
    n = reads.n_reads
    first, lens = reads.read_first_seq, np.diff(reads.seq_off.astype(np.int64))
    paired = [bool(reads.is_paired(r)) for r in range(n)]
    return O.first_it_restatement([lens[first[r]] for r in range(n)], [lens[first[r] + 1] if paired[r] else 0 for r in range(n)], paired)


def test_init_is_the_first_iterations_dict_of_a_mixed_store():
    rng = np.random.default_rng(5)
    seq = lambda n: ("".join("ACGT"[i] for i in rng.integers(0, 4, n)), "I" * n)
    reads = ReadSet.from_lists([seq(int(n)) for n in rng.integers(20, 200, 70)], [(seq(int(a)), seq(int(b))) for a, b in rng.integers(20, 200, (131, 2))])
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        sc.sr_originals_init()
        off, entries = sc.sr_originals_fetch()
        text = sc.sr_originals_text()
    want_off, want = O.to_csr(_first_dict(reads))
    assert off.tolist() == want_off.tolist() and entries.tobytes() == want.tobytes()
    assert text == host.sr_originals_text(want_off, want) and text.count(b"\n") == 201


def _second_iteration(sc, ref1, seed):
    """random tables over the new dict (the call reads nothing else of a merge call), first_it off: device, mirror and restatement"""
    n = len(ref1.off) - 1
    _, t2 = O.make_case(seed, n, [2, 3, 5, 17, 40, 2, 3], n_orig=4)
    maps1 = O.to_maps(ref1.off, ref1.entries)
    ref2 = host.sr_originals_next(ref1.off, ref1.entries, t2)
    dev2 = sc.sr_originals_next(t2, None, None, None)
    _same(dev2, sc.sr_originals_fetch(), sc.sr_originals_text(), ref2, "second iteration")
    want, status = O.next_restatement(maps1, t2)
    assert ref2.status.tolist() == status.tolist()
    O.assert_dict_equals_maps(ref2.off, ref2.entries, want, "second iteration")
    # the iteration did work: super-reads that own the originals of several reads
    assert ref2.n_entries > n / 2 and (np.diff(ref2.off.astype(np.int64)) >= 10).any()
    return ref2


@functools.lru_cache(maxsize=None)
def _clique_chain():
    g = CM.seeded_cliques()
    g["csr"] = EM.csr(g["V"], g["rows"])
    g["off"], g["nodes"] = SR.clique_csr(g["cliques"])
    return g


def test_a_real_clique_chain_and_a_second_iteration():
    g = _clique_chain()
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.sr_originals_init()
        sc.graph_load(*g["csr"])
        merged = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        nxt = sc.sr_clique_next(g["off"], g["nodes"], merged, g["vertex_read"], g["vertex_fwd"], keep_singletons=50)
        assert not nxt.empty and len(nxt.srs) > 50 and nxt.n_self_merged >= 0
        # the dict outlives the store it was made for: the call runs after hc_sr_clique_next has replaced the store
        dev = sc.sr_originals_next(nxt, merged, g["vertex_read"], g["vertex_fwd"], first_it=True)
        maps0 = _first_dict(g["reads"])
        ref = host.sr_originals_next(*O.to_csr(maps0), nxt, merged, g["vertex_read"], g["vertex_fwd"], first_it=True)
        _same(dev, sc.sr_originals_fetch(), sc.sr_originals_text(), ref, "clique chain")
        want, status = O.next_restatement(maps0, OR.tables_from(nxt, merged, g["vertex_read"], g["vertex_fwd"], True))
        assert not status.any() and dev.n_failed == 0 and len(dev.off) - 1 == nxt.new_read_count
        O.assert_dict_equals_maps(ref.off, ref.entries, want, "clique chain")
        # every original read that went into the new store is named once at least, a super-read names as many as its clique has vertices
        sizes = np.diff(dev.off.astype(np.int64))
        assert sizes.max() >= 40 and (sizes >= 1).all()
        _second_iteration(sc, ref, 31)


@functools.lru_cache(maxsize=None)
def _edge_chain():
    g = EM.seeded_graph()
    g["csr"] = EM.csr(g["V"], g["rows"])
    return g


def test_a_real_edge_merge_chain_with_self_merged_pairs_and_a_second_iteration():
    g = _edge_chain()
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.sr_originals_init()
        sc.graph_load(*g["csr"])
        pairs = sc.graph_merge_pairs()
        edge = sc.sr_edge_merge(pairs, g["vertex_read"], g["vertex_fwd"])
        nxt = sc.sr_merge_next(pairs, edge, g["vertex_read"], g["vertex_fwd"], keep_singletons=100)
        assert nxt.n_self_merged > 50 and nxt.n_trivials > 500
        dev = sc.sr_originals_next(nxt, edge, g["vertex_read"], g["vertex_fwd"], first_it=True)
        maps0 = _first_dict(g["reads"])
        ref = host.sr_originals_next(*O.to_csr(maps0), nxt, edge, g["vertex_read"], g["vertex_fwd"], first_it=True)
        _same(dev, sc.sr_originals_fetch(), sc.sr_originals_text(), ref, "edge chain")
        t = OR.tables_from(nxt, edge, g["vertex_read"], g["vertex_fwd"], True)
        want, status = O.next_restatement(maps0, t)
        assert not status.any()
        O.assert_dict_equals_maps(ref.off, ref.entries, want, "edge chain")
        # a self-merged pair's paired originals carry the shift of :938-949
        k = int(np.flatnonzero(nxt.pair_kind == MN.MN_SINGLE_SELF)[0])
        assert nxt.overlap_pos[k] > 0 and any(e["paired"] for e in want[int(nxt.pair_new_id[k])].values())
        _second_iteration(sc, ref, 32)


def test_refusals_leave_the_kept_dict_as_it_was():
    maps, t = O.make_case(2, 40, [2, 3, 5, 8])
    off, entries = O.to_csr(maps)
    with hc.EdgeScorer() as sc:
        with pytest.raises(hc.HcError, match="no read store") as e:
            sc.sr_originals_init()
        assert e.value.status == -5  # HC_ERR_STATE
        sc.set_reads(_dummy_reads(40))
        for call in (sc.sr_originals_fetch, sc.sr_originals_text, lambda: sc.sr_originals_next(t, None, None, None)):
            with pytest.raises(hc.HcError, match="no dict on the device") as e:
                call()
            assert e.value.status == -5
        with pytest.raises(hc.HcError, match="not the number of reads of the current store"):
            sc.sr_originals_load(off[:-1], entries)
        sc.sr_originals_load(off, entries)

        def unchanged():
            back = sc.sr_originals_fetch()
            assert back[0].tolist() == off.tolist() and back[1].tobytes() == entries.tobytes()

        with pytest.raises(hc.HcError, match="not the number of reads of the current store"):
            sc.sr_originals_load(np.concatenate([off, off[-1:]]), entries)
        bad = off.copy()
        bad[3], bad[4] = off[4] + 1, off[3]
        with pytest.raises(hc.HcError, match="descends"):
            sc.sr_originals_load(bad, entries)
        bad = off.copy()
        bad[0] = 1
        with pytest.raises(hc.HcError, match=r"orig_off\[0\] is not 0"):
            sc.sr_originals_load(bad, entries)
        e2 = entries[::-1].copy()
        with pytest.raises(hc.HcError, match="strictly ascend"):
            sc.sr_originals_load(off, e2)
        unchanged()
        for change, what in ((dict(new_read_count=3), "not below new_read_count"), (dict(vertex_read=t.vertex_read + 40), "no read of the kept dict"),
                             (dict(sr_clique=t.sr_clique + 9), "names no clique")):
            with pytest.raises(hc.HcError, match=what) as e:
                sc.sr_originals_next(OR.Tables(**{**t.__dict__, **change}), None, None, None)
            assert e.value.status == -1
            unchanged()
        with pytest.raises(hc.HcError, match="no text on the device"):
            from haploconduct_amd import _native as N

            N.check(N.lib.hc_sr_originals_text_fetch(sc._ctx, 0, 1, None), "hc_sr_originals_text_fetch")
        # and the call still works afterwards
        dev = sc.sr_originals_next(t, None, None, None)
        ref = host.sr_originals_next(off, entries, t)
        _same(dev, sc.sr_originals_fetch(), sc.sr_originals_text(), ref, "after the refusals")
