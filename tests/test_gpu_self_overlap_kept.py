"""The self-overlap merge from the consensus bytes kept on the device (hc_sr_merge_self_overlaps_kept, hc_sr_kept_load, hc_sr_kept_fetch;
include/hcsr.h) against the reference's golden vectors, the host mirror and the host-input device call: offsets, scores as bit patterns,
statuses, output offsets and the appended bytes, read back with hc_sr_kept_fetch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR
from haploconduct_amd import host, synth
from haploconduct_amd import next_reads as NR
from tests import _srself

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


def _kept(sc, seq, qual, pairs, **kw):
    """kept_load + the kept call; (result in the host-input form, the raw result)"""
    sc.sr_kept_load(seq, qual)
    r = sc.sr_merge_self_overlaps_kept(pairs, **kw)
    assert int(r.out_off[0]) == np.asarray(seq).size
    return r.relative(), r


@pytest.fixture(scope="module")
def batch():
    """300 pairs with mates of 16 .. 200 bases and the mirror's answer, computed once."""
    seq, qual, pairs, _ = _srself.make_batch(300, 16, 200, seed=505, max_overlap=60)
    return seq, qual, pairs, host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)


def test_kept_call_equals_every_golden_case():
    def run(seq, qual, pairs, settings, min_qual):
        with hc.EdgeScorer(settings) as sc:
            sc.sr_keep_device(True)
            return _kept(sc, seq, qual, pairs, min_qual=min_qual)[0]

    assert _srself.check_against_golden(run) >= 150


def test_mixed_batch_equals_the_mirror_and_the_host_input_call(batch):
    seq, qual, pairs, ref = batch
    merged = ref.status == SR.SR_SELF_MERGED
    assert merged.mean() >= 0.2 and (~merged).mean() >= 0.2, "a batch that is all one kind proves nothing"
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        rel, raw = _kept(sc, seq, qual, pairs)
        _srself.assert_same(rel, ref, "kept call against the mirror")
        _srself.assert_same(rel, sc.sr_merge_self_overlaps(seq, qual, pairs), "kept call against the host-input call")
        s, q = sc.sr_kept_fetch(0, seq.size)
        assert np.array_equal(s, seq) and np.array_equal(q, qual), "the original kept region changed"
        i = int(np.flatnonzero(merged)[3])
        assert raw.merged(i) == ref.merged(i) and raw.merged(int(np.flatnonzero(~merged)[0])) == (b"", b"")
    print(f"mixed batch: {pairs.size} pairs, {rel.n_merged} merged, host pairs {rel.n_host_pairs}, device {rel.ms_device:.3f} ms, host {rel.ms_host:.3f} ms")


# ---- the alignment sweep for the 16-byte loads ---------------------------------------------------------------------------
def _sweep_batch():
    """Mates of 1 .. 48 bases, each behind as few filler bytes (0 .. 15) as put off1 at residue i mod 16 and off2 at residue 5 i + 3: both take
    every residue.  The last mate ends at the last byte.  From 20 bases on mate 2 starts with mate 1's last 16 bases: those pairs merge."""
    rng = np.random.default_rng(16)
    s, q, pairs, at = [], [], np.zeros(48, SR.SR_PAIR_DTYPE), 0
    for i in range(48):
        l1, l2 = i + 1, (7 * i) % 48 + 1
        m1 = rng.choice(ACGT, l1)
        m2 = rng.choice(ACGT, l2)
        if l1 >= 20 and l2 >= 16:
            m2[:16] = m1[-16:]
        for k, m in enumerate((m1, m2)):
            fill = ((5 * i + 3 if k else i) - at) % 16
            s += [np.full(fill, ord("A"), np.uint8), m]
            q += [np.full(fill, 70, np.uint8), np.full(m.size, 70, np.uint8)]
            at += fill
            pairs[i]["off2" if k else "off1"], pairs[i]["len2" if k else "len1"] = at, m.size
            at += m.size
    seq, qual = np.concatenate(s), np.concatenate(q)
    assert set(int(x) % 16 for x in pairs["off1"]) == set(range(16)) == set(int(x) % 16 for x in pairs["off2"])
    assert int(pairs[-1]["off2"]) + int(pairs[-1]["len2"]) == seq.size
    return seq, qual, pairs


def _owners(pairs, at):
    return [i for i, P in enumerate(pairs) if any(int(P[o]) <= at < int(P[o]) + int(P[n]) for o, n in (("off1", "len1"), ("off2", "len2")))]


@pytest.fixture(scope="module")
def sweep():
    seq, qual, pairs = _sweep_batch()
    return seq, qual, pairs, host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=4)


def test_alignment_sweep_clean(sweep):
    seq, qual, pairs, clean = sweep
    assert (clean.status == SR.SR_SELF_MERGED).sum() >= 10 and (clean.status == SR.SR_SELF_NONE).sum() >= 10
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        _srself.assert_same(_kept(sc, seq, qual, pairs)[0], clean, "alignment sweep, clean")


@pytest.mark.parametrize("where", ["first", "last", "before", "after"])
@pytest.mark.parametrize("what", ["base", "qual_low", "qual_high"])
def test_alignment_sweep_with_one_invalid_symbol(sweep, where, what):
    """One invalid symbol per run, at the first or last byte of a mate or at the byte just before or behind it, for both mates of every pair:
    only the pairs that own the byte are refused (check_pair's answer, through the mirror), every other pair is what it is in the clean batch."""
    seq, qual, pairs, clean = sweep
    n_runs = 0
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        for i in range(pairs.size):
            for o, n in (("off1", "len1"), ("off2", "len2")):
                a, b = int(pairs[i][o]), int(pairs[i][o]) + int(pairs[i][n])
                at = {"first": a, "last": b - 1, "before": a - 1, "after": b}[where]
                if not 0 <= at < seq.size:
                    continue
                s, q = seq.copy(), qual.copy()
                if what == "base":
                    s[at] = ord("x")
                else:
                    q[at] = 32 if what == "qual_low" else 127
                own = _owners(pairs, at)
                assert i in own or where in ("before", "after")  # (behind mate 1 may lie mate 2 of the same pair: then the pair owns the byte)
                expect = clean.status.copy()
                expect[own] = SR.SR_SELF_BAD_SYMBOL
                mir = host.sr_merge_self_overlaps(s, q, pairs, n_threads=1)
                assert np.array_equal(mir.status, expect)
                rel, _ = _kept(sc, s, q, pairs)
                _srself.assert_same(rel, mir, f"pair {i} {o} {where} {what}")
                for j in range(pairs.size):
                    if j not in own:
                        assert rel.overlap_pos[j] == clean.overlap_pos[j] and rel.merged(j) == clean.merged(j)
                n_runs += 1
    assert n_runs >= 94


def test_bad_pairs_among_good_ones(batch):
    seq, qual, pairs, ref = batch
    n = 64
    cut = int(pairs[n]["off1"])
    s, q, p = seq[:cut].copy(), qual[:cut].copy(), pairs[:n].copy()
    q[int(p[5]["off1"]) + 3] = 127          # a quality byte outside [33,126]
    s[int(p[9]["off2"])] = ord("x")         # a base outside ACGTN
    q[int(p[20]["off2"]) + int(p[20]["len2"]) - 1] = 32
    p[30]["len1"] = 0
    p[31]["len2"] = 0
    p[40]["off2"] = cut - 3                 # mate 2 runs past the kept bytes
    p[45]["off1"] = 1 << 63
    p[50]["off2"] = cut                     # a mate that starts exactly at the kept size
    bad = {5: 3, 9: 3, 20: 3, 30: 2, 31: 2, 40: 2, 45: 2, 50: 2}
    mir = host.sr_merge_self_overlaps(s, q, p, n_threads=4)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        rel, _ = _kept(sc, s, q, p)
    _srself.assert_same(rel, mir, "bad pairs among good ones")
    for i in range(n):
        if i in bad:
            assert rel.status[i] == bad[i] and rel.overlap_pos[i] == -1 and rel.merged(i) == (b"", b"")
        else:  # the neighbours are what they are in the clean batch
            assert rel.status[i] == ref.status[i] and rel.overlap_pos[i] == ref.overlap_pos[i] and rel.merged(i) == ref.merged(i)


@pytest.mark.parametrize("n_values", [94, 6])
def test_quality_alphabets(n_values):
    """The batches of test_gpu_self_overlap.py::test_quality_alphabets — 94 values: the log table stays in device memory, 6: it sits in LDS —
    and, with 6, a seventh value that occurs only in a pair the check refuses: it takes no part in the tables, as on the host."""
    vals = np.arange(33, 127, dtype=np.uint8) if n_values == 94 else np.array([60, 64, 66, 68, 70, 71], np.uint8)
    w = np.ones(vals.size) if n_values == 6 else np.where(vals >= 65, 30.0, 1.0)
    seq, qual, pairs, _ = _srself.make_batch(300, 16, 200, seed=n_values, qvals=vals, qweights=w / w.sum(), max_overlap=60)
    assert np.unique(qual).size == n_values
    ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        rel, _ = _kept(sc, seq, qual, pairs)
        _srself.assert_same(rel, ref, f"{n_values} quality values")
        assert 0.1 < rel.n_merged / pairs.size < 0.9
        if n_values == 6:
            s, q = seq.copy(), qual.copy()
            q[int(pairs[7]["off1"]) + 2] = 100  # a valid value, but only here ...
            s[int(pairs[7]["off2"])] = ord("x")  # ... in a pair with an invalid base
            q[int(pairs[11]["off1"])] = 101
            p = pairs.copy()
            p[11]["len2"] = 0                   # ... and in a pair that is refused unread
            mir = host.sr_merge_self_overlaps(s, q, p, n_threads=16)
            assert mir.status[7] == SR.SR_SELF_BAD_SYMBOL and mir.status[11] == SR.SR_SELF_BAD_PAIR
            _srself.assert_same(_kept(sc, s, q, p)[0], mir, "a quality value of a refused pair alone")


@pytest.mark.parametrize("n_pairs,length", [(64, 700), (1, 3000)])
def test_long_mates(n_pairs, length):
    """700 bases: several chunks of offsets with the mates resident in LDS; 3,000 bases: the windowed path."""
    vals, w = _srself.quality_alphabet()
    keep = vals >= 45
    seq, qual, pairs, _ = _srself.make_batch(n_pairs, length, length, seed=length, overlap_frac=1.0 if n_pairs == 1 else 0.5, sub_rate=0.0, qvals=vals[keep],
                                             qweights=w[keep] / w[keep].sum())
    ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        rel, _ = _kept(sc, seq, qual, pairs)
    _srself.assert_same(rel, ref, f"{n_pairs} x {length}")
    assert rel.n_merged >= max(1, n_pairs // 4)


DRIVER = r"""
import numpy as np
import haploconduct_amd as hc
from haploconduct_amd import host
from tests import _srself
seq, qual, pairs, rejected = _srself.band_batch(-10)
ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
with hc.EdgeScorer() as sc:
    sc.sr_keep_device(True)
    sc.sr_kept_load(seq, qual)
    raw = sc.sr_merge_self_overlaps_kept(pairs)
    rel = raw.relative()
    _srself.assert_same(rel, ref, "wide band, kept call")
    s, q = sc.sr_kept_fetch(0, seq.size)
    assert np.array_equal(s, seq) and np.array_equal(q, qual)
    print("host pairs", rel.n_host_pairs, "of", pairs.size, "merged", rel.n_merged, "rejected", int(rejected.sum()), "merged lower",
          int((rejected & (ref.overlap_pos > 0)).sum()))
"""


def test_band_path_with_a_widened_guard_band():
    """HC_SR_SELF_BAND_LOG2=-10 (a test knob) sends hundreds of pairs to the host: their mates come back through the
    gather, their merged reads go up packed and are spliced in behind the kept bytes.  A process of its own: the knob is read from the
    environment."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DRIVER], cwd=root, env=dict(os.environ, HC_SR_SELF_BAND_LOG2="-10"), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    w = r.stdout.split()
    n_host, n_pairs, n_merged, n_lower = (int(w[w.index(k) + 1]) for k in ("pairs", "of", "merged", "lower"))
    assert 0 < n_host < n_pairs and n_lower >= 8 and n_merged > n_lower, r.stdout


def _edge_layouts(n_reads=3000, n_cand=1200):
    """The layouts of test_gpu_self_overlap.py::test_round_trip_from_sr_consensus: two members each, layouts 2 i and 2 i + 1 the mates of pair i."""
    reads, meta = synth.make_single_dataset(n_reads, 6000, seed=61)
    cand = synth.single_candidates(meta, min_overlap=60, n_candidates=n_cand, seed=62)
    e = np.zeros(cand.size, host.EDGE_DTYPE)
    for k in ("read1", "read2", "ori1", "ori2", "pos1"):
        e[k] = cand[k]
    e["v1"] = cand["read1"].astype(np.uint64) + np.where(cand["ori1"] != 0, 0, reads.n_reads).astype(np.uint64)
    e["v2"] = cand["read2"].astype(np.uint64) + np.where(cand["ori2"] != 0, 0, reads.n_reads).astype(np.uint64)
    layouts, members = host.sr_edge_layouts(e, reads)
    return reads, layouts, members


def _pairs_of(out_off):
    n = (out_off.size - 1) // 2
    pairs = np.zeros(n, SR.SR_PAIR_DTYPE)
    pairs["off1"], pairs["off2"] = out_off[0:2 * n:2], out_off[1:2 * n:2]
    pairs["len1"] = (out_off[1:2 * n:2] - out_off[0:2 * n:2]).astype(np.uint32)
    pairs["len2"] = (out_off[2:2 * n + 1:2] - out_off[1:2 * n:2]).astype(np.uint32)
    return pairs


def test_growth_and_succession():
    """About 20 KB of 2 x 150 mates of which most merge: the appended bytes exceed the headroom of an eighth, so the kept buffers grow with
    their contents.  A second call appends behind the first and reads what the first appended; a consensus call then resets the kept bytes."""
    seq, qual, pairs, _ = synth.make_mate_pairs(68, 150, 150, seed=9, qvals=np.array([70, 73], np.uint8), qweights=np.array([0.5, 0.5]), sub_rate=0.0,
                                                overlap_frac=1.0, max_overlap=60)
    ref1 = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    assert 20000 <= seq.size <= 21000 and ref1.merged_seq.size > seq.size // 8 + 16 and ref1.n_merged >= 60
    reads, layouts, members = _edge_layouts(400, 40)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        rel1, raw1 = _kept(sc, seq, qual, pairs)
        _srself.assert_same(rel1, ref1, "first call")
        end1 = int(raw1.out_off[-1])
        assert end1 == seq.size + ref1.merged_seq.size == SR.kept_size(sc._ctx)
        # second call: mate 1 = a read the first call appended, mate 2 = the original mate 2 of the same pair (it overlaps the merged read's end)
        m = np.flatnonzero(ref1.status == SR.SR_SELF_MERGED)[:40]
        p2 = np.zeros(m.size, SR.SR_PAIR_DTYPE)
        p2["off1"], p2["len1"] = raw1.out_off[m], (raw1.out_off[m + 1] - raw1.out_off[m]).astype(np.uint32)
        p2["off2"], p2["len2"] = pairs["off2"][m], pairs["len2"][m]
        all_seq, all_qual = np.concatenate([seq, ref1.merged_seq]), np.concatenate([qual, ref1.merged_qual])
        ref2 = host.sr_merge_self_overlaps(all_seq, all_qual, p2, n_threads=16)
        assert ref2.n_merged >= 30
        raw2 = sc.sr_merge_self_overlaps_kept(p2)
        assert int(raw2.out_off[0]) == end1 and SR.kept_size(sc._ctx) == end1 + ref2.merged_seq.size
        _srself.assert_same(raw2.relative(), ref2, "second call")
        s, q = sc.sr_kept_fetch(0, end1)
        assert np.array_equal(s, all_seq) and np.array_equal(q, all_qual), "earlier kept bytes changed"
        cons = sc.sr_consensus(layouts, members)
        assert cons.cons_seq.size > 0 and SR.kept_size(sc._ctx) == cons.cons_seq.size
        s, q = sc.sr_kept_fetch()
        assert np.array_equal(s, cons.cons_seq) and np.array_equal(q, cons.cons_qual)


def test_round_trip_from_sr_consensus_to_the_next_store():
    """hc_sr_consensus with keeping on -> the kept call on its bytes -> hc_sr_set_next_reads naming the merged reads as consensus bytes at
    out_off -> the new store's raw arrays: what the mirrors give for cons || merged."""
    reads, layouts, members = _edge_layouts()
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        cons = sc.sr_consensus(layouts, members)
        pairs = _pairs_of(cons.out_off)
        raw = sc.sr_merge_self_overlaps_kept(pairs)
        ref = host.sr_merge_self_overlaps(cons.cons_seq, cons.cons_qual, pairs, n_threads=16)
        assert int(raw.out_off[0]) == cons.cons_seq.size
        _srself.assert_same(raw.relative(), ref, "round trip")
        merged = raw.status == SR.SR_SELF_MERGED
        assert pairs.size >= 500 and merged.sum() >= 1 and (~merged).sum() >= 5  # (these layouts' mates seldom overlap: a few pairs merge)
        singles = [NR.single(int(raw.out_off[i]), int(raw.out_off[i + 1] - raw.out_off[i])) for i in np.flatnonzero(merged)]
        paired = [NR.paired(int(P["off1"]), int(P["len1"]), int(P["off2"]), int(P["len2"])) for P in pairs[~merged]]
        entries = np.array(singles + paired, NR.NEXT_ENTRY_DTYPE)
        dev = sc.sr_set_next_reads(entries)
        got = sc.sr_next_reads_fetch()
    want = NR.host_next_reads(reads, np.concatenate([cons.cons_seq, ref.merged_seq]), np.concatenate([cons.cons_qual, ref.merged_qual]), entries)
    assert not dev.empty and np.array_equal(dev.status, want.status) and np.array_equal(dev.new_id, want.new_id)
    assert (dev.status[:len(singles)] == NR.NEXT_KEPT).sum() >= 1 and (dev.status[len(singles):] == NR.NEXT_KEPT).sum() >= 100
    for k in ("read_first_seq", "seq_off", "bases", "quals"):
        assert np.array_equal(getattr(got, k), getattr(want.reads, k)), k


def test_state_errors_and_the_empty_call(batch):
    seq, qual, pairs, _ = batch
    import ctypes as C
    st = SR.make_self_settings()
    n = pairs.size
    pos, score, status, off, n_out, kept = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), C.c_uint64(0), C.c_uint64(9)

    def call(sc, k):
        return N.lib.hc_sr_merge_self_overlaps_kept(sc._ctx, pairs.ctypes.data, k, C.byref(st), pos.ctypes.data, score.ctypes.data, status.ctypes.data,
                                                    off.ctypes.data, C.byref(n_out), None)

    err_state = None
    with hc.EdgeScorer() as sc:
        err_state = N.lib.hc_sr_set_next_reads(sc._ctx, None, 0, None, None, 0, C.byref(N.hc_sr_next_settings(0, 0)), None, None, None)  # HC_ERR_STATE
        assert err_state != 0
        assert call(sc, n) == err_state, "keeping off"
        assert N.lib.hc_sr_kept_load(sc._ctx, seq.ctypes.data, qual.ctypes.data, seq.size) == err_state
        sc.sr_keep_device(True)
        assert call(sc, n) == err_state, "keeping on, nothing kept"
        assert N.lib.hc_sr_kept_fetch(sc._ctx, 0, 0, None, None, C.byref(kept)) == err_state and kept.value == 0
        sc.sr_kept_load(seq[:0], qual[:0])   # kept, and empty
        assert SR.kept_size(sc._ctx) == 0 and call(sc, 0) == 0 and off[0] == 0
        assert call(sc, 4) == 0 and (status[:4] == SR.SR_SELF_BAD_PAIR).all() and n_out.value == 0
        sc.sr_kept_load(seq, qual)
        assert call(sc, 0) == 0 and off[0] == seq.size and n_out.value == 0
        buf = np.zeros(16, np.uint8)
        rc = N.lib.hc_sr_kept_fetch(sc._ctx, seq.size - 8, 16, buf.ctypes.data, buf.ctypes.data, C.byref(kept))
        assert rc not in (0, err_state) and kept.value == seq.size and not buf.any(), "a range outside the kept bytes is HC_ERR_ARG"
        assert N.lib.hc_sr_kept_fetch(sc._ctx, seq.size + 1, 0, None, None, C.byref(kept)) == rc
        with pytest.raises(N.HcError):
            sc.sr_kept_fetch(seq.size - 8, 16)
        s, q = sc.sr_kept_fetch(seq.size - 8, 8)
        assert np.array_equal(s, seq[-8:]) and np.array_equal(q, qual[-8:])
