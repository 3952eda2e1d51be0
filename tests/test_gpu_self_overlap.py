"""The self-overlap merge on the device (hc_sr_merge_self_overlaps, include/hcsr.h) against the reference's golden vectors, against the
host mirror at sizes no golden file holds — offsets, scores as bit patterns, statuses, output offsets and merged bytes — and, independently
of the mirror, against the oracle's overlap_score."""
import os
import subprocess
import sys

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import consensus as SR
from haploconduct_amd import host, synth
from tests import _srself

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch():
    """2,000 pairs with mates of 16 .. 300 bases, 1 % substitutions, the quality alphabet of the SAVAGE example reads; about half overlap by
    15 .. 60 bases by construction (longer overlaps seldom stay free of substitutions, and one costs the merge).  The mirror's answer is
    computed once."""
    seq, qual, pairs, over = _srself.make_batch(2000, 16, 300, seed=101, max_overlap=60)
    ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    return seq, qual, pairs, over, ref


def test_device_equals_every_golden_case():
    def run(seq, qual, pairs, settings, min_qual):
        with hc.EdgeScorer(settings) as sc:
            return sc.sr_merge_self_overlaps(seq, qual, pairs, min_qual=min_qual)

    assert _srself.check_against_golden(run) >= 150


def test_mixed_batch_equals_the_mirror(batch):
    seq, qual, pairs, over, ref = batch
    merged = ref.status == SR.SR_SELF_MERGED
    assert merged.mean() >= 0.25 and (~merged).mean() >= 0.25, "a batch that is all one kind proves nothing"
    with hc.EdgeScorer() as sc:
        dev = sc.sr_merge_self_overlaps(seq, qual, pairs)
        _srself.assert_same(dev, ref, "mixed batch")
        again = sc.sr_merge_self_overlaps(seq, qual, pairs, count_first=True)  # cap = 0, then fetch; the context's tables are reused
        _srself.assert_same(again, ref, "count-then-fetch")
    print(f"mixed batch: {pairs.size} pairs, {dev.n_merged} merged, {dev.n_offsets} offsets, host pairs {dev.n_host_pairs}, device {dev.ms_device:.3f} ms")


def test_scores_equal_the_oracle_independently_of_the_mirror(batch, oracle):
    seq, qual, pairs, over, _ = batch
    with hc.EdgeScorer() as sc:
        dev = sc.sr_merge_self_overlaps(seq[:int(pairs[200]["off1"])], qual[:int(pairs[200]["off1"])], pairs[:200])
    n_hit = 0
    for i in range(200):
        P = pairs[i]
        s1, q1 = seq[P["off1"]:P["off1"] + P["len1"]].tobytes(), qual[P["off1"]:P["off1"] + P["len1"]].tobytes()
        s2, q2 = seq[P["off2"]:P["off2"] + P["len2"]].tobytes(), qual[P["off2"]:P["off2"] + P["len2"]].tobytes()
        stop = int(dev.overlap_pos[i]) if dev.overlap_pos[i] > 0 else 0
        for p in range(int(P["len1"]) - 15, stop, -1):
            assert oracle.overlap_score(s1, s2, q1, q2, p)["score"] <= 0.99, (i, p)
        if stop:
            sc_ref = oracle.overlap_score(s1, s2, q1, q2, stop)["score"]
            assert sc_ref > 0.99 and np.float64(sc_ref).view(np.uint64) == dev.score[i:i + 1].view(np.uint64)[0], (i, stop)
            n_hit += 1
    assert 50 <= n_hit <= 150


@pytest.mark.parametrize("n_pairs,length", [(64, 700), (1, 3000)])
def test_long_mates(n_pairs, length):
    """700 bases: several chunks of offsets with the mates resident in LDS; 3,000 bases: the windowed path."""
    assert (length > 2048) == (length == 3000)
    vals, w = _srself.quality_alphabet()
    keep = vals >= 45  # (without Phred 0 and no substitutions: overlaps of hundreds of bases merge)
    seq, qual, pairs, _ = _srself.make_batch(n_pairs, length, length, seed=length, overlap_frac=1.0 if n_pairs == 1 else 0.5, sub_rate=0.0, qvals=vals[keep],
                                             qweights=w[keep] / w[keep].sum())
    ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    with hc.EdgeScorer() as sc:
        dev = sc.sr_merge_self_overlaps(seq, qual, pairs)
    _srself.assert_same(dev, ref, f"{n_pairs} x {length}")
    assert dev.n_merged >= max(1, n_pairs // 4)
    if n_pairs == 1:  # the hit's overlap is longer than one window of 1,024 positions; then the same mates apart: the whole windowed scan
        assert min(length - int(dev.overlap_pos[0]), length) > 1024
        pairs2 = pairs.copy()
        seq2 = seq.copy()
        seq2[length:] = np.random.default_rng(3).choice(np.frombuffer(b"ACGT", np.uint8), length)
        ref2 = host.sr_merge_self_overlaps(seq2, qual, pairs2, n_threads=16)
        with hc.EdgeScorer() as sc:
            dev2 = sc.sr_merge_self_overlaps(seq2, qual, pairs2)
        _srself.assert_same(dev2, ref2, "windowed, nothing merges")
        assert dev2.n_merged == 0


@pytest.mark.parametrize("n_values", [94, 6])
def test_quality_alphabets(n_values):
    """94 values: the log table (two triangles of 96 rows, 74,496 bytes) stays in device memory; 6 values: it sits in LDS beside the mates."""
    vals = np.arange(33, 127, dtype=np.uint8) if n_values == 94 else np.array([60, 64, 66, 68, 70, 71], np.uint8)
    w = np.ones(vals.size) if n_values == 6 else np.where(vals >= 65, 30.0, 1.0)
    seq, qual, pairs, _ = _srself.make_batch(300, 16, 200, seed=n_values, qvals=vals, qweights=w / w.sum(), max_overlap=60)
    assert np.unique(qual).size == n_values
    ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    with hc.EdgeScorer() as sc:
        dev = sc.sr_merge_self_overlaps(seq, qual, pairs)
    _srself.assert_same(dev, ref, f"{n_values} quality values")
    assert 0.1 < dev.n_merged / pairs.size < 0.9


DRIVER = r"""
import sys
import numpy as np
import haploconduct_amd as hc
from haploconduct_amd import host
from tests import _srself
seq, qual, pairs, rejected = _srself.band_batch(-10)
ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
with hc.EdgeScorer() as sc:
    dev = sc.sr_merge_self_overlaps(seq, qual, pairs)
    _srself.assert_same(dev, ref, "wide band, offsets around min_score")
    print("host pairs", dev.n_host_pairs, "of", pairs.size, "merged", dev.n_merged, "rejected", int(rejected.sum()), "merged lower",
          int((rejected & (ref.overlap_pos > 0)).sum()))
    seq, qual, pairs, _ = _srself.make_batch(400, 16, 300, seed=77, max_overlap=60)
    _srself.assert_same(sc.sr_merge_self_overlaps(seq, qual, pairs), host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16), "wide band, mixed batch")
"""


def test_band_path_with_a_widened_guard_band():
    """HC_SR_SELF_BAND_LOG2=-10 (a test knob) widens the guard band around ln(min_score) to 2^-10: offsets whose x falls
    inside go to the host's libm, and the result is unchanged.  The batch (_srself.band_batch) is built so that deciding offsets fall inside
    the band on both sides of 0.99: where the host rejects one, its scan has to go on below the offset the device reported — to no merge in
    most such pairs, to a merge at a smaller offset in eight built for it.  A process of its own: the knob is read from the environment."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DRIVER], cwd=root, env=dict(os.environ, HC_SR_SELF_BAND_LOG2="-10"), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    w = r.stdout.split()
    n_host, n_pairs, n_merged, n_rejected, n_lower = (int(w[w.index(k) + 1]) for k in ("pairs", "of", "merged", "rejected", "lower"))
    assert n_lower >= 8 and n_rejected > n_lower, r.stdout  # the continuation of scan_pair ran, to a smaller offset and to none
    assert n_rejected <= n_host < n_pairs and n_merged > n_lower, r.stdout  # every rejection went through the host; the device decided pairs alone too


def test_statuses_and_edge_calls(batch):
    seq, qual, pairs, over, ref = batch
    n = 64
    cut = int(pairs[n]["off1"])
    s, q, p = seq[:cut].copy(), qual[:cut].copy(), pairs[:n].copy()
    q[int(p[5]["off1"]) + 3] = 127          # a quality byte outside [33,126]
    s[int(p[9]["off2"])] = ord("x")         # a base outside ACGTN
    q[int(p[20]["off2"]) + int(p[20]["len2"]) - 1] = 32
    p[30]["len1"] = 0
    p[31]["len2"] = 0
    p[40]["off2"] = cut - 3                 # mate 2 runs past n_bytes
    bad = {5: 3, 9: 3, 20: 3, 30: 2, 31: 2, 40: 2}
    mir = host.sr_merge_self_overlaps(s, q, p, n_threads=4)
    with hc.EdgeScorer() as sc:
        dev = sc.sr_merge_self_overlaps(s, q, p)
        _srself.assert_same(dev, mir, "bad pairs among good ones")
        for i in range(n):
            if i in bad:
                assert dev.status[i] == bad[i] and dev.overlap_pos[i] == -1 and dev.merged(i) == (b"", b"")
            else:  # the neighbours are what they are in the clean batch
                assert dev.status[i] == ref.status[i] and dev.overlap_pos[i] == ref.overlap_pos[i] and dev.merged(i) == ref.merged(i)
        none = sc.sr_merge_self_overlaps(s, q, p[:0])
        assert none.out_off.tolist() == [0] and none.merged_seq.size == 0 and none.n_merged == 0
        # cap = 0: everything but the bytes, and the size to come back with
        import ctypes as C
        from haploconduct_amd import _native as N
        st = SR.make_self_settings(n_threads=4)
        pos, score, status, off, n_out = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), C.c_uint64(0)
        rc = N.lib.hc_sr_merge_self_overlaps(sc._ctx, s.ctypes.data, q.ctypes.data, s.size, p.ctypes.data, n, C.byref(st), pos.ctypes.data, score.ctypes.data,
                                             status.ctypes.data, off.ctypes.data, None, None, 0, C.byref(n_out), None)
        assert rc != 0 and n_out.value == dev.merged_seq.size > 0
        assert np.array_equal(pos, dev.overlap_pos) and np.array_equal(off, dev.out_off) and np.array_equal(status, dev.status)


def test_round_trip_from_sr_consensus():
    """hc_sr_consensus on layouts of two members each; its cons_seq / cons_qual / out_off go straight into the new call as mates (layouts 2 i
    and 2 i + 1 are the mates of pair i)."""
    reads, meta = synth.make_single_dataset(3000, 6000, seed=61)
    cand = synth.single_candidates(meta, min_overlap=60, n_candidates=1200, seed=62)
    e = np.zeros(cand.size, host.EDGE_DTYPE)
    for k in ("read1", "read2", "ori1", "ori2", "pos1"):
        e[k] = cand[k]
    e["v1"] = cand["read1"].astype(np.uint64) + np.where(cand["ori1"] != 0, 0, reads.n_reads).astype(np.uint64)
    e["v2"] = cand["read2"].astype(np.uint64) + np.where(cand["ori2"] != 0, 0, reads.n_reads).astype(np.uint64)
    layouts, members = host.sr_edge_layouts(e, reads)
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        cons = sc.sr_consensus(layouts, members)
        n = layouts.size // 2
        pairs = np.zeros(n, SR.SR_PAIR_DTYPE)
        pairs["off1"], pairs["off2"] = cons.out_off[0:2 * n:2], cons.out_off[1:2 * n:2]
        pairs["len1"] = (cons.out_off[1:2 * n:2] - cons.out_off[0:2 * n:2]).astype(np.uint32)
        pairs["len2"] = (cons.out_off[2:2 * n + 1:2] - cons.out_off[1:2 * n:2]).astype(np.uint32)
        dev = sc.sr_merge_self_overlaps(cons.cons_seq, cons.cons_qual, pairs)
    ref = host.sr_merge_self_overlaps(cons.cons_seq, cons.cons_qual, pairs, n_threads=16)
    _srself.assert_same(dev, ref, "round trip")
    assert n >= 500 and (pairs["len1"] > 0).mean() > 0.9 and np.unique(cons.cons_qual).size > 6
    print(f"round trip: {n} pairs, {dev.n_merged} merged, {np.unique(cons.cons_qual).size} quality values")


def _same_columns(n_values, n_pairs=64, min_overlap=5):
    """Single-end reads (A_0, B_0, A_1, ...) of 33 .. 70 symbols, the pairs (A_i, B_i) over their packed bytes, and the two-member layouts
    {A_i at 0, B_i at p} with p = len1 - min_overlap, the first offset of the scan.  Every tenth base is an N; B_i starts with A_i's
    last min_overlap bases, each replaced by a random one with probability 1/2, so the shared columns agree, disagree and hold Ns."""
    from haploconduct_amd.readstore import ReadSet
    rng = np.random.default_rng(1000 + n_values)
    qvals = np.array([60, 64, 66, 68, 70, 71], np.uint8) if n_values == 6 else np.arange(35, 35 + n_values, dtype=np.uint8)
    singles = []
    for _ in range(n_pairs):
        a, b = (rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(n), p=[0.225] * 4 + [0.1]) for n in rng.integers(33, 71, 2))
        keep = rng.random(min_overlap) < 0.5
        b[:min_overlap][keep] = a[-min_overlap:][keep]
        singles += [(x.tobytes(), rng.choice(qvals, x.size).tobytes()) for x in (a, b)]
    reads = ReadSet.from_lists(singles=singles)
    assert np.unique(reads.quals).size == n_values
    off = reads.seq_off
    pairs = np.zeros(n_pairs, SR.SR_PAIR_DTYPE)
    pairs["off1"], pairs["off2"] = off[0:-1:2], off[1:-1:2]
    pairs["len1"], pairs["len2"] = off[1::2] - off[0:-1:2], off[2::2] - off[1:-1:2]
    p = pairs["len1"].astype(np.int32) - min_overlap
    members = np.zeros(2 * n_pairs, SR.SR_MEMBER_DTYPE)
    members["read"] = np.arange(2 * n_pairs)
    members["pos"][1::2] = p
    layouts = np.zeros(n_pairs, SR.SR_LAYOUT_DTYPE)
    layouts["first_member"], layouts["n_members"], layouts["total_len"] = 2 * np.arange(n_pairs), 2, pairs["len2"].astype(np.int32) + p
    return reads, pairs, p, layouts, members


def _assert_same_columns(merged, cons, reads, pairs, p, min_qual):
    assert (merged.status == SR.SR_SELF_MERGED).all() and np.array_equal(merged.overlap_pos, p)
    assert (cons.status == SR.SR_OK).all() and (cons.ret == 0).all()
    assert np.array_equal(merged.out_off, cons.out_off) and merged.out_off[-1] == (pairs["len2"] + p).sum()
    assert np.array_equal(merged.merged_seq, cons.cons_seq) and np.array_equal(merged.merged_qual, cons.cons_qual)
    # The shared columns in which two called bases of comparable quality disagree: 'N' / '$' at min_qual 0.99, a base at 0.0.  (Phred values
    # at most 10 apart: the better base's share of the total probability is then at most 10 / 11, whatever the two values are.)
    n_disagree = n_masked = 0
    for i, P in enumerate(pairs):
        at1, at2, n = int(P["off1"]) + int(p[i]), int(P["off2"]), int(P["len1"]) - int(p[i])
        a, b = reads.bases[at1:at1 + n], reads.bases[at2:at2 + n]
        out = merged.merged_seq[int(merged.out_off[i]) + int(p[i]):int(merged.out_off[i]) + int(P["len1"])]
        differ = (a != b) & (a != ord("N")) & (b != ord("N")) & (np.abs(reads.quals[at1:at1 + n].astype(int) - reads.quals[at2:at2 + n]) <= 10)
        n_disagree += int(differ.sum())
        n_masked += int((out[differ] == ord("N")).sum())
    assert n_disagree >= 32 and n_masked == (n_disagree if min_qual == 0.99 else 0)


@pytest.mark.parametrize("min_qual", [0.99, 0.0])
@pytest.mark.parametrize("n_values", [6, 40])
def test_merge_and_consensus_write_the_same_columns(n_values, min_qual):
    """Both kernels finish a column with hc_sr_column.h.  With min_score < 0 every pair merges at its first offset p = len1 - min_overlap;
    hc_sr_consensus on {A_i at 0, B_i at p}, total_len = len2 + p, without error correction, has to write the same bytes at the same
    offsets.  6 quality values: the store's fused 8-bit symbols; 40: its wide ones.  Columns of one member (both ends), of two, Ns in both."""
    reads, pairs, p, layouts, members = _same_columns(n_values)
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        merged = sc.sr_merge_self_overlaps(reads.bases, reads.quals, pairs, min_score=-1.0, min_qual=min_qual, min_overlap=5)
        cons = sc.sr_consensus(layouts, members, min_qual=min_qual)
    _assert_same_columns(merged, cons, reads, pairs, p, min_qual)
