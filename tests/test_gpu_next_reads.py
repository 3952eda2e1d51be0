"""hc_sr_set_next_reads on the device (include/hcsr.h) against the host mirror: the raw arrays of the new store byte for byte, and the new
store itself against a second context that takes the mirror's arrays through hc_set_reads — hc_get_info, scoring records and consensus
output identical.  The kept consensus bytes (hc_sr_keep_device) against the bytes hc_sr_consensus returned, host-finished columns included."""
import ctypes as C

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR
from haploconduct_amd import host, synth
from haploconduct_amd import next_reads as NR
from haploconduct_amd.readstore import ReadSet
from haploconduct_amd.records import OVERLAP_DTYPE
from tests import _sr

pytestmark = pytest.mark.gpu

EDGE_LENS = [1, 15, 16, 17, 63, 64, 65, 2049]


def _rand_seq(rng, n, quals, p_n=0.02):
    b = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n, p=[(1 - p_n) / 4] * 4 + [p_n])
    return b.tobytes(), rng.choice(np.asarray(quals, np.uint8), n).tobytes()


def _store(rng, quals, n_singles=90, n_pairs=60):
    """Singles and pairs of every length of EDGE_LENS and of 20..200 bases otherwise; a few reads with too many N."""
    lens = EDGE_LENS + [int(x) for x in rng.integers(20, 200, n_singles - len(EDGE_LENS))]
    singles = [_rand_seq(rng, n, quals, rng.choice([0.0, 0.02, 0.08], p=[0.3, 0.5, 0.2])) for n in lens]
    pl = [(a, b) for a, b in zip(EDGE_LENS, EDGE_LENS[::-1])] + [(int(a), int(b)) for a, b in rng.integers(20, 160, (n_pairs - len(EDGE_LENS), 2))]
    pairs = [(_rand_seq(rng, a, quals), _rand_seq(rng, b, quals, rng.choice([0.0, 0.1]))) for a, b in pl]
    return ReadSet.from_lists(singles, pairs)


def _entries(rng, reads, cons, extra_len, n, kinds=(0, 1, 2, 3), bad=True, srcs=(NR.SRC_CONSENSUS, NR.SRC_BYTES)):
    """n entries of the kinds given, in the writers' order (singles, trivials, pairs), from both sources, with odd offsets, the lengths of
    EDGE_LENS where the source is long enough, empty mates and — bad = True — a few entries that are refused.  srcs: the sources the
    super-reads' mates are drawn from."""
    first = reads.read_first_seq.astype(np.int64)
    is_pair = (first[1:] - first[:-1]) == 2
    room = {NR.SRC_CONSENSUS: int(cons.out_off[-1]), NR.SRC_BYTES: extra_len}

    def piece(i):
        src = int(rng.choice(srcs))
        if src == NR.SRC_CONSENSUS and rng.random() < 0.5 and cons.out_off.size > 1:  # a whole layout's bytes
            l = int(rng.integers(0, cons.out_off.size - 1))
            return int(cons.out_off[l]), int(cons.out_off[l + 1] - cons.out_off[l]), src
        ln = EDGE_LENS[i % len(EDGE_LENS)] if rng.random() < 0.5 else int(rng.integers(0, 300))
        ln = min(ln, room[src])
        off = int(rng.integers(0, room[src] - ln + 1)) | (1 if ln < room[src] else 0)
        return min(off, room[src] - ln), ln, src

    out = {k: [] for k in (0, 1, 2, 3)}
    for i in range(n):
        k = kinds[i % len(kinds)]
        if k == NR.NEXT_SINGLE:
            out[k].append(NR.single(*piece(i)))
        elif k == NR.NEXT_PAIRED:
            (o1, l1, s1), (o2, l2, s2) = piece(i), piece(i + 3)
            out[k].append(NR.paired(o1, l1, o2, l2, s1, s2))
        else:
            pool = np.flatnonzero(is_pair == (k == NR.NEXT_TRIVIAL_PAIRED))
            out[k].append(NR.trivial(int(pool[i % pool.size]) if rng.random() < 0.7 else int(rng.choice(pool)), bool(rng.integers(0, 2)), k == 3))
    if bad:
        out[0] += [NR.single(3, 0), NR.single(room[0], 1), NR.single(0, 5, 2)]
        out[1] += [NR.paired(0, 5, 9, 0), NR.paired(1, 0, 9, 7, 1, 0)]
        out[2] += [NR.trivial(reads.n_reads), NR.trivial(int(np.flatnonzero(is_pair)[0])), (0, 0, 0, 0, 0, NR.NEXT_TRIVIAL, 0, 0, 3)]
        out[1] += [NR.paired(0, 4, 1, room[1], 0, 1)]
    trivials = sorted(out[2] + out[3], key=lambda e: e[4])  # vertex order
    return np.array(out[0] + trivials + out[1], NR.NEXT_ENTRY_DTYPE)


def _candidates(rng, reads, n):
    first = reads.read_first_seq.astype(np.int64)
    is_pair = (first[1:] - first[:-1]) == 2
    lens = (reads.seq_off[1:] - reads.seq_off[:-1]).astype(np.int64)
    rec = []
    for pool, ordc in ((np.flatnonzero(~is_pair), ord("-")), (np.flatnonzero(is_pair), ord("1"))):
        if pool.size < 2:
            continue
        r = np.zeros(n, OVERLAP_DTYPE)
        a = pool[rng.integers(0, pool.size, n)]
        b = pool[(np.searchsorted(pool, a) + rng.integers(1, pool.size, n)) % pool.size]
        r["read1"], r["read2"], r["ord"] = a, b, ordc
        r["pos1"] = rng.integers(0, lens[first[a]])
        if ordc != ord("-"):
            r["pos2"] = rng.integers(0, np.minimum(lens[first[a] + 1], lens[first[b] + 1]))
        r["ori1"], r["ori2"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
        rec.append(r)
    return np.concatenate(rec) if rec else np.zeros(0, OVERLAP_DTYPE)


def _same_readset(a, b, what):
    assert np.array_equal(a.read_first_seq, b.read_first_seq), what + ": read_first_seq differs"
    assert np.array_equal(a.seq_off, b.seq_off), what + ": seq_off differs"
    assert np.array_equal(a.bases, b.bases), what + ": bases differ"
    assert np.array_equal(a.quals, b.quals), what + ": quals differ"


def _equivalence(seed, quals, n_entries, kinds=(0, 1, 2, 3), bad=True, keep_singletons=30, expect_K=None, srcs=(NR.SRC_CONSENSUS, NR.SRC_BYTES)):
    rng = np.random.default_rng(seed)
    reads = _store(rng, quals)
    layouts, members = _sr.random_cliques(rng, reads, 120, 1, 6)
    ex_seq, ex_qual = _rand_seq(rng, 4000, quals, 0.03)
    with hc.EdgeScorer() as sc, hc.EdgeScorer() as sc2:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        cons = sc.sr_consensus(layouts, members, min_clique_size=1)
        assert cons.out_off[-1] > 2000
        entries = _entries(rng, reads, cons, len(ex_seq), n_entries, kinds, bad, srcs)
        ex = (np.frombuffer(ex_seq, np.uint8), np.frombuffer(ex_qual, np.uint8))
        ref = NR.host_next_reads(reads, cons.cons_seq, cons.cons_qual, entries, *ex, keep_singletons=keep_singletons)
        dev = sc.sr_set_next_reads(entries, *ex, keep_singletons=keep_singletons)
        assert np.array_equal(dev.status, ref.status) and np.array_equal(dev.new_id, ref.new_id)
        for k in ("n_kept", "n_dropped_empty", "n_dropped_n_rate", "n_dropped_short", "n_bad", "n_seq", "n_bytes"):
            assert dev.counts[k] == ref.counts[k], k
        assert dev.empty == ref.empty
        if ref.empty:
            _same_readset(sc.sr_next_reads_fetch(), reads, "the old store stays")
            return dev, ref
        got = sc.sr_next_reads_fetch()
        _same_readset(got, ref.reads, "new raw arrays")
        sc2.set_reads(ref.reads)
        assert sc.info() == sc2.info() and sc.kernel_info() == sc2.kernel_info()
        assert np.array_equal(sc.locality_order(), sc2.locality_order())
        if expect_K is not None:
            assert sc.info()["qual_alphabet"] == expect_K
        cand = hc.EdgeScorer.pack_cands(_candidates(np.random.default_rng(seed + 1), ref.reads, 3000))
        if cand.size:
            assert sc.score_cands(cand).tobytes() == sc2.score_cands(cand).tobytes()
        l2, m2 = _sr.random_cliques(np.random.default_rng(seed + 2), ref.reads, 60, 1, 5)
        _sr.assert_same(sc.sr_consensus(l2, m2, min_clique_size=1), sc2.sr_consensus(l2, m2, min_clique_size=1), "consensus over the new reads")
        return dev, ref


def test_equivalence_with_the_mirror_and_with_a_store_loaded_from_its_arrays():
    dev, ref = _equivalence(1, synth.QUAL_SET, 400)
    st = set(ref.status.tolist())
    assert st == {NR.NEXT_KEPT, NR.NEXT_DROPPED_EMPTY, NR.NEXT_DROPPED_N_RATE, NR.NEXT_DROPPED_SHORT, NR.NEXT_BAD_ENTRY}
    first = ref.reads.read_first_seq.astype(np.int64)
    assert {1, 2} == set((first[1:] - first[:-1]).tolist())


# The quality alphabet of the RESULT decides its encoding: narrow (K <= 6, <= 30), the two wide 8-bit ones (31..48, 49..60), 16-bit.  The
# consensus writes quality values of its own making, so here the super-reads' bytes come from the call's extra bytes (and the trivials from
# the store): the result's alphabet is then the K values the test chose.  The consensus source is covered by the other tests.
@pytest.mark.parametrize("K", [5, 24, 40, 55, 70])
def test_every_encoding_of_the_resulting_store(K):
    quals = [33 + q for q in np.linspace(2, 93, K).round().astype(int)] if K > 42 else [35 + q for q in range(K)]
    assert len(set(quals)) == K
    dev, ref = _equivalence(100 + K, quals, 300, bad=False, expect_K=K, srcs=(NR.SRC_BYTES,))
    assert np.unique(ref.reads.quals).size == K  # (every value survives into the new store)
    with hc.EdgeScorer() as sc:
        sc.set_reads(ref.reads)
        assert sc.info()["qual_alphabet"] == K


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_entry_counts_around_a_wave(n):
    _equivalence(200 + n, synth.QUAL_SET, n, bad=False, keep_singletons=0)


def test_only_trivials_and_a_second_iteration_from_the_new_store():
    rng = np.random.default_rng(7)
    reads = _store(rng, synth.QUAL_SET)
    first = reads.read_first_seq.astype(np.int64)
    is_pair = (first[1:] - first[:-1]) == 2
    entries = np.array([NR.trivial(r, bool(r % 3 == 0), bool(is_pair[r])) for r in range(reads.n_reads)], NR.NEXT_ENTRY_DTYPE)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        ref = NR.host_next_reads(reads, None, None, entries, keep_singletons=16)
        dev = sc.sr_set_next_reads(entries, keep_singletons=16)
        assert np.array_equal(dev.status, ref.status) and np.array_equal(dev.new_id, ref.new_id) and 0 < ref.counts["n_kept"] < reads.n_reads
        _same_readset(sc.sr_next_reads_fetch(), ref.reads, "trivials only")
        # again, from the new store: every read reversed
        r1 = ref.reads
        p1 = (r1.read_first_seq[1:].astype(np.int64) - r1.read_first_seq[:-1]) == 2
        e2 = np.array([NR.trivial(r, True, bool(p1[r])) for r in range(r1.n_reads)], NR.NEXT_ENTRY_DTYPE)
        ref2 = NR.host_next_reads(r1, None, None, e2)
        dev2 = sc.sr_set_next_reads(e2)
        assert np.array_equal(dev2.status, ref2.status) and (ref2.status == NR.NEXT_KEPT).all()
        _same_readset(sc.sr_next_reads_fetch(), ref2.reads, "second iteration")


def test_a_batch_in_which_every_entry_is_dropped_leaves_the_store():
    rng = np.random.default_rng(9)
    reads = _store(rng, synth.QUAL_SET)
    ex = np.frombuffer(b"N" * 40 + b"ACGT", np.uint8)
    entries = np.array([NR.single(1, 39, NR.SRC_BYTES), NR.single(3, 0, NR.SRC_BYTES), NR.trivial(reads.n_reads), NR.trivial(0),
                        NR.paired(0, 4, 40, 0, 1, 1), NR.single(0, 1)], NR.NEXT_ENTRY_DTYPE)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        info = sc.info()
        dev = sc.sr_set_next_reads(entries, ex, np.full(ex.size, 70, np.uint8), keep_singletons=10 ** 6)
        ref = NR.host_next_reads(reads, None, None, entries, ex, np.full(ex.size, 70, np.uint8), keep_singletons=10 ** 6)
        assert dev.empty and ref.empty and np.array_equal(dev.status, ref.status) and (dev.new_id == -1).all()
        assert dev.status.tolist() == [2, 1, 4, 3, 1, 4]
        assert sc.info() == info
        _same_readset(sc.sr_next_reads_fetch(), reads, "the old store stays")


def test_kept_consensus_bytes_include_the_host_finished_columns():
    """Deep layouts, as tests/test_gpu_consensus.py builds them from reads that tile one place of a genome: host threads finish a share of
    the columns, and the scatter launch writes them into the kept bytes.  (Cliques of reads that disagree would do for the patch, but
    their consensus holds more than 5 % N and one entry over all of it would not pass the N rate.)"""
    reads, meta = synth.make_single_dataset(3000, 7500, flip_frac=0.0, n_strains=1, seed=71)
    rng = np.random.default_rng(72)
    order = np.argsort(meta["s"], kind="stable")
    n_l, depth = 1500, 12
    idx = order[rng.integers(0, reads.n_reads - depth, n_l)[:, None] + np.arange(depth)[None, :]]
    pos = meta["s"][idx] - meta["s"][idx][:, :1]
    members = np.zeros(n_l * depth, SR.SR_MEMBER_DTYPE)
    members["read"], members["pos"] = idx.ravel(), pos.ravel()
    layouts = np.zeros(n_l, SR.SR_LAYOUT_DTYPE)
    layouts["first_member"], layouts["n_members"], layouts["total_len"] = np.arange(n_l) * depth, depth, (pos + 150).max(axis=1)
    for kw in (dict(error_correction=True, min_clique_size=4), dict(error_correction=False, min_qual=0.9)):
        with hc.EdgeScorer() as sc:
            sc.sr_keep_device(True)
            sc.set_reads(reads)
            cons = sc.sr_consensus(layouts, members, **kw)
            n = int(cons.out_off[-1])
            print(f"{kw}: {n} columns, host-finished {cons.n_host_columns}")
            assert cons.n_host_columns > 0 and n > 0
            dev = sc.sr_set_next_reads(np.array([NR.single(0, n)], NR.NEXT_ENTRY_DTYPE))
            assert not dev.empty and dev.status.tolist() == [NR.NEXT_KEPT]
            got = sc.sr_next_reads_fetch()
            assert np.array_equal(got.bases, cons.cons_seq) and np.array_equal(got.quals, cons.cons_qual)


def test_keeping_off_changes_nothing_and_the_new_call_is_a_state_error():
    reads, meta = synth.make_paired_dataset(300, 1500, flip_frac=0.25, seed=11)
    cand = hc.EdgeScorer.pack_cands(synth.paired_candidates(meta, n_candidates=1500, seed=12))
    layouts, members = _sr.random_cliques(np.random.default_rng(13), reads, 300, 1, 12)
    entries = np.array([NR.trivial(0, is_paired=True)], NR.NEXT_ENTRY_DTYPE)
    with hc.EdgeScorer() as off, hc.EdgeScorer() as on:
        on.sr_keep_device(True)
        for sc in (off, on):
            sc.set_reads(reads)
        assert off.info() == on.info()
        assert off.score_cands(cand).tobytes() == on.score_cands(cand).tobytes()
        a, b = off.sr_consensus(layouts, members, error_correction=True), on.sr_consensus(layouts, members, error_correction=True)
        _sr.assert_same(a, b, "keeping on / off")
        _sr.assert_same(a, host.sr_consensus(reads, layouts, members, error_correction=True), "keeping off against the mirror")
        with pytest.raises(N.HcError) as e:
            off.sr_set_next_reads(entries)
        assert e.value.status == -5  # HC_ERR_STATE
        with pytest.raises(N.HcError) as e:
            off.sr_next_reads_fetch()
        assert e.value.status == -5
        # turned on after hc_set_reads: there are no kept raw arrays yet
        off.sr_keep_device(True)
        with pytest.raises(N.HcError) as e:
            off.sr_set_next_reads(entries)
        assert e.value.status == -5
        # turned off again: what was kept is released, the store and its results stay
        on.sr_keep_device(False)
        with pytest.raises(N.HcError):
            on.sr_set_next_reads(entries)
        assert off.score_cands(cand).tobytes() == on.score_cands(cand).tobytes()


def test_a_regular_result_takes_the_locality_order():
    """Reads of one length, singles only: the new store is `regular` and gets its locality order, as hc_set_reads gives it."""
    reads, meta = synth.make_single_dataset(700, 2000, seed=21, n_rate=0.0)
    entries = np.array([NR.trivial(r, bool(r % 2)) for r in range(0, reads.n_reads, 2)], NR.NEXT_ENTRY_DTYPE)
    ref = NR.host_next_reads(reads, None, None, entries)
    with hc.EdgeScorer() as sc, hc.EdgeScorer() as sc2:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        dev = sc.sr_set_next_reads(entries)
        assert (dev.status == NR.NEXT_KEPT).all() and np.array_equal(dev.new_id, ref.new_id)
        _same_readset(sc.sr_next_reads_fetch(), ref.reads, "regular result")
        sc2.set_reads(ref.reads)
        order = sc.locality_order()
        assert order.size == ref.reads.n_reads and np.array_equal(order, sc2.locality_order())
        assert sc.info() == sc2.info() and sc.kernel_info(10 ** 7) == sc2.kernel_info(10 ** 7)
        cand = hc.EdgeScorer.pack_cands(_candidates(np.random.default_rng(22), ref.reads, 4000))
        assert sc.score_cands(cand).tobytes() == sc2.score_cands(cand).tobytes()
