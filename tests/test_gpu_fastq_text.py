"""hc_sr_fastq_write_text / hc_sr_fastq_text_fetch on the device (include/hcsr.h) against the host mirrors, byte for byte, files and counts:
stores whose sequence lengths sit on every head, tail and vector boundary of the wave's copy, ids of every digit count up to five (every
alignment of a record's start), empty files, fetches by pieces, the tips of the store a next-store call READ — through hc_sr_set_next_reads
alone and through hc_sr_edge_merge -> hc_sr_merge_next on the seeded chain of tests/test_gpu_merge_next.py —, the store left in place by
HC_SR_NEXT_EMPTY, a store straight from hc_set_reads, the state errors, and the other calls of the context unaffected."""
import ctypes as C

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import fastq_text as FQ
from haploconduct_amd import host
from haploconduct_amd import next_reads as NR
from tests import _fastq_text as T
from tests import _merge_next as M
from tests.test_gpu_merge_next import _chain
from tests.test_gpu_next_reads import _candidates, _same_readset

pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200, 1023, 1024, 1025, 3000]
ERR_ARG, ERR_STATE = -1, -5


def _mirror(store, tip_store=None, tip_reads=()):
    """-> the four files as the mirrors write them"""
    return [host.sr_fastq_text(store, f) for f in range(3)] + [host.sr_fastq_tips_text(tip_store if tip_store is not None else store, tip_reads)]


def _n_records(store, tip_store=None, tip_reads=()):
    paired = np.diff(store.read_first_seq.astype(np.int64)) == 2
    ts = tip_store if tip_store is not None else store
    return [int((~paired).sum()), int(paired.sum()), int(paired.sum()), sum(2 if ts.is_paired(int(r)) else 1 for r in tip_reads)]


def _check(got, want, n_records, what=""):
    for f, name in enumerate(FQ.FILES):
        assert got["n_bytes"][f] == len(want[f]), (what, name, got["n_bytes"][f], len(want[f]))
        if got[name] != want[f]:
            a, b = np.frombuffer(got[name], np.uint8), np.frombuffer(want[f], np.uint8)
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{what}: {name} differs first at byte {at}: {got[name][max(0, at - 20):at + 20]!r} != {want[f][max(0, at - 20):at + 20]!r}")
    assert got["n_records"] == n_records, (what, got["n_records"], n_records)
    assert got["ms_device"] > 0


def _status(fn, *a):
    with pytest.raises(hc.HcError) as e:
        fn(*a)
    return e.value.status


@pytest.mark.parametrize("kind", ["single", "paired", "mixed"])
def test_every_boundary_of_the_copy(kind):
    """3 000 takes the wave more than one pass; the other lengths put the head, the tail and the vectors of both copies on every side of 16
    and of a wave's 1 024 bytes; the shuffled order and the ids' digits move the records' starts"""
    rng = np.random.default_rng({"single": 1, "paired": 2, "mixed": 3}[kind])
    lens = LENS * 3 + rng.integers(1, 70, 30).tolist()
    rng.shuffle(lens)
    store = T.make_store(rng, lens, kind)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(store)
        tips = rng.integers(0, store.n_reads, 40)  # no next-store call ran: the tips are reads of this store
        got = sc.sr_fastq_text(tips, np.arange(store.n_reads))
        _check(got, _mirror(store, None, tips), _n_records(store, None, tips), kind)
        assert got["singles"] == T.store_files(store)[0] and got["tips"] == T.tips_file(store, tips.tolist())  # (and the restatement)


def test_ids_of_every_digit_count_put_the_records_on_every_alignment():
    rng = np.random.default_rng(4)
    store = T.make_store(rng, [20] * 10001, "single")
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(store)
        got = sc.sr_fastq_text()
    want = _mirror(store)
    _check(got, want, [10001, 0, 0, 0], "10 001 reads of 20")
    starts = np.cumsum([0] + [len(str(r)) + 46 for r in range(10000)])
    assert set((starts % 16).tolist()) == set(range(16))  # every destination alignment occurred
    assert got["singles"].endswith(b"\n") and got["singles"].count(b"\n@10000\n") == 1


@pytest.mark.parametrize("kind", ["single", "paired"])
def test_empty_files_and_fetches_by_pieces(kind):
    rng = np.random.default_rng(5)
    store = T.make_store(rng, rng.integers(1, 90, 64).tolist(), kind)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(store)
        cn = FQ.write_text(sc._ctx)
        want = _mirror(store)
        empty = [1, 2, 3] if kind == "single" else [0, 3]
        for f in range(4):
            assert cn.n_bytes[f] == len(want[f]) and (cn.n_bytes[f] == 0) == (f in empty) and (cn.n_records[f] == 0) == (f in empty)
            assert FQ.fetch(sc._ctx, f, 0, 0) == b"" and FQ.fetch(sc._ctx, f, cn.n_bytes[f], 0) == b""  # count 0 is OK, also at the end
            assert _status(FQ.fetch, sc._ctx, f, 0, cn.n_bytes[f] + 1) == ERR_ARG
            assert _status(FQ.fetch, sc._ctx, f, cn.n_bytes[f] + 1, 0) == ERR_ARG
            assert N.lib.hc_sr_fastq_text_fetch(sc._ctx, f, 1 << 63, 1 << 63, None) == ERR_ARG  # (first + count wraps)
        assert _status(FQ.fetch, sc._ctx, 4, 0, 0) == ERR_ARG
        for f in (0,) if kind == "single" else (1, 2):
            n, text = int(cn.n_bytes[f]), want[f]
            rec0 = text.index(b"\n@") + 1  # the second record's first byte
            cuts = sorted({0, 3, rec0 - 2, rec0, rec0 + 1, n // 2, n - 1, n})  # inside a record, across a boundary, at it
            pieces = [FQ.fetch(sc._ctx, f, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
            assert b"".join(pieces) == text
            assert FQ.fetch(sc._ctx, f, rec0 - 5, 12) == text[rec0 - 5:rec0 + 7]


def test_tips_are_reads_of_the_store_hc_sr_set_next_reads_read():
    rng = np.random.default_rng(6)
    old = T.make_store(rng, LENS[:11] + rng.integers(20, 120, 80).tolist(), "mixed", with_n=False)
    n = old.n_reads
    vertex_read = rng.permutation(n).astype(np.uint32)
    tips = rng.choice(n, 17, replace=False).astype(np.uint32)  # vertices
    tip_reads = vertex_read[tips]
    assert len({old.is_paired(int(r)) for r in tip_reads}) == 2
    keep = [r for r in range(n) if r not in set(tip_reads.tolist())]
    entries = np.array([NR.trivial(r, rev=bool(k % 3 == 0), is_paired=old.is_paired(r)) for k, r in enumerate(keep)], NR.NEXT_ENTRY_DTYPE)
    ref = NR.host_next_reads(old, None, None, entries)
    assert not ref.empty and ref.reads.n_reads == len(keep)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(old)
        res = sc.sr_set_next_reads(entries)
        assert not res.empty
        got = sc.sr_fastq_text(tips, vertex_read)
        _check(got, _mirror(ref.reads, old, tip_reads), _n_records(ref.reads, old, tip_reads), "after hc_sr_set_next_reads")
        none = sc.sr_fastq_text()  # n_tips = 0 with NULL pointers
        assert none["tips"] == b"" and none["n_records"][3] == 0 and none["singles"] == got["singles"]


def test_tips_through_edge_merge_and_merge_next_on_the_chain():
    g = _chain()
    reads = g["reads"]
    rng = np.random.default_rng(8)
    tip_flags = (rng.random(reads.n_reads) < 0.1).astype(np.uint8)
    kw = dict(keep_singletons=100, store_tips_separately=True, tip_reads=tip_flags)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        sc.graph_load(*g["csr"])
        pairs = sc.graph_merge_pairs()
        edge = sc.sr_edge_merge(pairs, g["vertex_read"], g["vertex_fwd"])
        ref = host.sr_merge_next(reads, edge.result.cons_seq, edge.result.cons_qual, pairs, edge, g["vertex_read"], g["vertex_fwd"], **kw)
        dev = sc.sr_merge_next(pairs, edge, g["vertex_read"], g["vertex_fwd"], **kw)
        assert not dev.empty and np.array_equal(dev.tips, ref.tips) and dev.tips.size > 20
        tip_reads = np.asarray(g["vertex_read"])[dev.tips]
        assert len({reads.is_paired(int(r)) for r in tip_reads}) == 2 and len({int(np.asarray(g["vertex_fwd"])[v]) for v in dev.tips}) == 2
        got = sc.sr_fastq_text(dev.tips, g["vertex_read"])
        # the tips: the OLD store's reads, forward whatever the vertex; files 0 - 2: the mirror's NEW arrays
        _check(got, _mirror(ref.reads, reads, tip_reads), _n_records(ref.reads, reads, tip_reads), "chain")
        assert got["n_records"][0] + got["n_records"][1] == dev.new_read_count and got["n_records"][0] >= dev.n_singles and got["n_records"][1] >= dev.n_paired
        none = sc.sr_fastq_text()
        assert none["tips"] == b"" and none["n_bytes"][3] == 0 and none["paired2"] == got["paired2"]


def test_tips_when_every_vertex_is_a_tip_come_from_the_store_in_place():
    c = M.make_case(3, 20, 0)
    n = c.reads.n_reads
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(c.reads)
        sc.sr_kept_load(c.cons_seq, c.cons_qual)
        res = sc.sr_merge_next(c.pairs, M.empty_edge(), c.vertex_read, c.vertex_fwd, store_tips_separately=True, tip_reads=np.ones(n, np.uint8))
        # HC_SR_NEXT_EMPTY, the store stays: every vertex is a tip but the few whose read fails test_N_rate first (src/SRBuilder.cpp:1292)
        assert res.empty and res.n_trivials == 0 and res.tips.size >= len(c.vertex_read) - 4
        tip_reads = np.asarray(c.vertex_read)[res.tips]
        got = sc.sr_fastq_text(res.tips, c.vertex_read)
        _check(got, _mirror(c.reads, None, tip_reads), _n_records(c.reads, None, tip_reads), "every vertex a tip")


def test_the_last_iteration_a_store_straight_from_hc_set_reads():
    rng = np.random.default_rng(9)
    store = T.make_store(rng, rng.integers(100, 2500, 60).tolist(), "mixed")
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(store)
        _check(sc.sr_fastq_text(), _mirror(store), _n_records(store), "no tips")
        tips = np.array([5, 0, 5, 11], np.uint32)
        vr = np.arange(store.n_reads, dtype=np.uint32)[::-1].copy()
        _check(sc.sr_fastq_text(tips, vr), _mirror(store, None, vr[tips]), _n_records(store, None, vr[tips]), "tips of the store itself")


def test_state_errors_leave_the_text_and_the_store_as_they_were():
    rng = np.random.default_rng(10)
    a = T.make_store(rng, rng.integers(30, 90, 40).tolist(), "mixed", with_n=False)
    ident = np.arange(a.n_reads, dtype=np.uint32)
    with hc.EdgeScorer() as sc:
        # keeping is off
        sc.set_reads(a)
        assert _status(sc.sr_fastq_text) == ERR_STATE
        assert _status(FQ.fetch, sc._ctx, 0, 0, 0) == ERR_STATE
        sc.sr_keep_device(True)
        assert _status(sc.sr_fastq_text) == ERR_STATE  # (this store's raw arrays were not kept)
        sc.set_reads(a)
        first = sc.sr_fastq_text([1, 2], ident)
        want_a = _mirror(a, None, [1, 2])
        _check(first, want_a, _n_records(a, None, [1, 2]), "before the errors")

        def still_there():
            for f in range(4):
                assert FQ.fetch(sc._ctx, f, 0, len(want_a[f])) == want_a[f]
            _same_readset(sc.sr_next_reads_fetch(), a, "the store after a refused call")

        # a tip vertex out of range; vertex_read beyond the store
        assert _status(sc.sr_fastq_text, [1, a.n_reads], ident) == ERR_ARG
        still_there()
        assert _status(sc.sr_fastq_text, [0, 3], np.array([0, 1, 2, a.n_reads], np.uint32)) == ERR_ARG
        still_there()
        cn = FQ.hc_sr_fastq_counts()
        assert N.lib.hc_sr_fastq_write_text(sc._ctx, None, 2, None, 0, C.byref(cn)) == ERR_ARG  # tips named, no arrays
        still_there()
        # a next-store call replaces the store: the text made from the old arrays is gone, the tips are the old store's
        keep_a = list(range(0, a.n_reads, 2))
        e1 = np.array([NR.trivial(r, is_paired=a.is_paired(r)) for r in keep_a], NR.NEXT_ENTRY_DTYPE)
        b = NR.host_next_reads(a, None, None, e1).reads
        assert not sc.sr_set_next_reads(e1).empty
        assert _status(FQ.fetch, sc._ctx, 0, 0, 0) == ERR_STATE
        last = a.n_reads - 1
        assert last >= b.n_reads
        tips1 = sc.sr_fastq_text([last], ident)  # a read of a, not of b
        assert tips1["tips"] == host.sr_fastq_tips_text(a, [last]) and tips1["singles"] == host.sr_fastq_text(b, 0)
        # a second next-store call overwrites the traded blocks: a is gone for good, and the tips are reads of the store THAT call read (b)
        e2 = np.array([NR.trivial(r, is_paired=b.is_paired(r)) for r in range(0, b.n_reads, 2)], NR.NEXT_ENTRY_DTYPE)
        c = NR.host_next_reads(b, None, None, e2).reads
        assert not sc.sr_set_next_reads(e2).empty
        assert _status(FQ.fetch, sc._ctx, 3, 0, 0) == ERR_STATE
        assert _status(sc.sr_fastq_text, [last], ident) == ERR_ARG  # the first call's table names a read the store that is there does not have
        assert _status(sc.sr_fastq_text, [b.n_reads], ident) == ERR_ARG
        tips2 = sc.sr_fastq_text([b.n_reads - 1, 0], ident)
        _check(tips2, _mirror(c, b, [b.n_reads - 1, 0]), _n_records(c, b, [b.n_reads - 1, 0]), "after the second call")
        # an empty call reads the store in place
        assert sc.sr_set_next_reads(np.zeros(0, NR.NEXT_ENTRY_DTYPE)).empty
        assert _status(sc.sr_fastq_text, [c.n_reads], ident) == ERR_ARG
        assert sc.sr_fastq_text([c.n_reads - 1], ident)["tips"] == host.sr_fastq_tips_text(c, [c.n_reads - 1])
        # hc_set_reads replaces the arrays: a fetch of the old text is refused, and the traded blocks are forgotten
        sc.set_reads(a)
        assert _status(FQ.fetch, sc._ctx, 0, 0, 0) == ERR_STATE
        assert sc.sr_fastq_text([last], ident)["tips"] == host.sr_fastq_tips_text(a, [last])
        # keeping goes off: everything goes
        sc.sr_keep_device(False)
        assert _status(FQ.fetch, sc._ctx, 0, 0, 0) == ERR_STATE
        assert _status(sc.sr_fastq_text) == ERR_STATE


def test_the_other_calls_of_the_context_are_unaffected():
    rng = np.random.default_rng(11)
    store = T.make_store(rng, rng.integers(100, 151, 300).tolist(), "mixed", with_n=False)
    cand = hc.EdgeScorer.pack_cands(_candidates(np.random.default_rng(3), store, 500))
    entries = np.array([NR.trivial(r, rev=bool(r % 2), is_paired=store.is_paired(r)) for r in range(0, store.n_reads, 3)], NR.NEXT_ENTRY_DTYPE)
    vr = np.arange(store.n_reads, dtype=np.uint32)
    with hc.EdgeScorer() as sc, hc.EdgeScorer() as plain:  # `plain` never writes text
        for s in (sc, plain):
            s.sr_keep_device(True)
            s.set_reads(store)
        sc.sr_fastq_text([3, 4], vr)
        _same_readset(sc.sr_next_reads_fetch(), plain.sr_next_reads_fetch(), "hc_sr_next_reads_fetch after the write")
        assert sc.score_cands(cand).tobytes() == plain.score_cands(cand).tobytes()
        assert sc.info() == plain.info()
        r1, r2 = sc.sr_set_next_reads(entries), plain.sr_set_next_reads(entries)
        assert np.array_equal(r1.new_id, r2.new_id) and np.array_equal(r1.status, r2.status)
        assert {k: v for k, v in r1.counts.items() if not k.startswith("ms_")} == {k: v for k, v in r2.counts.items() if not k.startswith("ms_")}
        sc.sr_fastq_text([1, 2, 5], vr)
        new = plain.sr_next_reads_fetch()
        _same_readset(sc.sr_next_reads_fetch(), new, "the new store after the write")
        cand2 = hc.EdgeScorer.pack_cands(_candidates(np.random.default_rng(4), new, 500))
        assert sc.score_cands(cand2).tobytes() == plain.score_cands(cand2).tobytes()
        assert sc.info() == plain.info() and sc.kernel_info() == plain.kernel_info()
