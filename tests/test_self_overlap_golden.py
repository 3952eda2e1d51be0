"""The host mirror of the self-overlap merge (hc_host_sr_merge_self_overlaps, include/hcsr.h) against the reference's own
merge_self_overlap (tests/golden/self_overlap.json, written by make_golden_self_overlap.py): merged or not, the offset and the merged
strings, byte for byte; and the mirror's own contract (statuses, count-then-fetch, threads)."""
import json

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR
from haploconduct_amd import host
from tests import _srself


def test_mirror_equals_every_golden_case():
    def run(seq, qual, pairs, settings, min_qual):
        return host.sr_merge_self_overlaps(seq, qual, pairs, settings, min_qual=min_qual, n_threads=3)

    assert _srself.check_against_golden(run) >= 150


def test_golden_file_holds_the_cases_it_should():
    g = json.load(open(_srself.GOLDEN))["cases"]
    names = {c["name"].split("/")[0] for c in g}
    for want in ("l1_14_hit_p1", "l1_15_hit_p1", "l1_16_hit_p1", "l1_17_hit_p1", "offsets_63_none", "offsets_64_p1", "offsets_65_pmax", "offsets_128_mid",
                 "offsets_129_none", "l2_1", "contained", "two_offsets", "n_run_both", "n_inside_hit", "mismatch_setting_loq", "min_read_len", "min_qual",
                 "all_phred", "savage_0_true", "savage_0_mates"):
        assert want in names, want
    merged = sum(c["merged"] for c in g)
    assert 0.25 * len(g) < merged < 0.75 * len(g)
    assert any(c["merged"] and len(c["merged_seq"]) < len(c["seq1"]) for c in g)  # the truncated output of a contained mate 2
    assert {c["mismatch"] for c in g} >= {0.0, 0.01} and {c["min_qual"] for c in g} >= {0.9, 0.99}
    # one case and its twin differ only in a setting and in the outcome
    for a, b in (("mismatch_setting_loq/mm0.0/mrl0/mq0.99", "mismatch_setting_loq/mm0.3/mrl0/mq0.99"), ("min_read_len/mm0.0/mrl80/mq0.99", "min_read_len/mm0.0/mrl81/mq0.99")):
        by = {c["name"]: c for c in g}
        assert by[a]["merged"] == 1 and by[b]["merged"] == 0, (a, b)


def test_scores_are_the_oracles(oracle):
    """independent of the mirror's own arithmetic: the score at the reported offset is the oracle's overlap_score there, above 0.99, and every
    larger offset scores at most 0.99"""
    seq, qual, pairs, _ = _srself.make_batch(60, 16, 200, seed=5, max_overlap=60)
    r = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=2)
    assert 10 < r.n_merged < 50
    for i in range(pairs.size):
        P = pairs[i]
        s1, q1 = seq[P["off1"]:P["off1"] + P["len1"]].tobytes(), qual[P["off1"]:P["off1"] + P["len1"]].tobytes()
        s2, q2 = seq[P["off2"]:P["off2"] + P["len2"]].tobytes(), qual[P["off2"]:P["off2"] + P["len2"]].tobytes()
        stop = int(r.overlap_pos[i]) if r.overlap_pos[i] > 0 else 0
        for p in range(int(P["len1"]) - 15, stop, -1):
            assert oracle.overlap_score(s1, s2, q1, q2, p)["score"] <= 0.99
        if stop:
            sc = oracle.overlap_score(s1, s2, q1, q2, stop)["score"]
            assert sc > 0.99 and np.float64(sc).view(np.uint64) == r.score[i:i + 1].view(np.uint64)[0]


def test_statuses_and_edge_calls():
    good = (b"ACGTACGTACGTACGTACGTAGG", b"I" * 23, b"GTACGTACGTACGTAGGTTT", b"I" * 20)
    mates = [good, (b"ACGTACGTACGTACGTACGTAGG", b"I" * 22 + b"\x7f", b"GTACGTACGTACGTAGGTTT", b"I" * 20), good, (b"ACGTACGTACGTACGTACGTAGG", b"I" * 23, b"GTACGTACxTACGTAGGTTT", b"I" * 20),
             good, (b"ACGTACGTACGTACGTACGTAGG", b"I" * 22 + b" ", b"GTACGTACGTACGTAGGTTT", b"I" * 20), good]
    seq, qual, pairs = SR.pack_pairs(mates)
    pairs = np.concatenate([pairs, np.zeros(4, SR.SR_PAIR_DTYPE)])
    pairs[7] = (0, 23, 0, 20)                  # len1 == 0
    pairs[8] = (0, 23, 23, 0)                  # len2 == 0
    pairs[9] = (seq.size - 5, 0, 10, 5)        # mate 1 runs past n_bytes
    pairs[10] = (0, 2**63, 23, 20)             # mate 2 starts far outside
    r = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=2)
    assert list(r.status) == [1, 3, 1, 3, 1, 3, 1, 2, 2, 2, 2]
    assert list(r.overlap_pos) == [6, -1, 6, -1, 6, -1, 6, -1, -1, -1, -1]
    assert all(r.merged(i) == r.merged(0) for i in (2, 4, 6)) and r.merged(0)[0] == b"ACGTACGTACGTACGTACGTAGGTTT"
    assert all(r.merged(i) == (b"", b"") for i in (1, 3, 5, 7, 8, 9, 10)) and r.n_merged == 4
    # no pairs; count-then-fetch equals the one-call form
    e = host.sr_merge_self_overlaps(seq, qual, pairs[:0])
    assert e.out_off.tolist() == [0] and e.merged_seq.size == 0
    c = host.sr_merge_self_overlaps(seq, qual, pairs, count_first=True)
    assert np.array_equal(c.merged_seq, r.merged_seq) and np.array_equal(c.out_off, r.out_off)
    n_out = N.C.c_uint64(0)
    st = SR.make_self_settings()
    cs = N.hc_settings()
    pos, sc, status, off = np.zeros(11, np.int32), np.zeros(11), np.zeros(11, np.uint32), np.zeros(12, np.uint64)
    rc = N.lib.hc_host_sr_merge_self_overlaps(N.C.byref(cs), seq.ctypes.data, qual.ctypes.data, seq.size, pairs.ctypes.data, 11, N.C.byref(st), pos.ctypes.data,
                                              sc.ctypes.data, status.ctypes.data, off.ctypes.data, None, None, 0, N.C.byref(n_out), None)
    assert rc != 0 and n_out.value == 4 * 26 and off.tolist() == r.out_off.tolist() and pos.tolist() == r.overlap_pos.tolist()


@pytest.mark.parametrize("min_score,min_overlap", [(-1.0, 15), (0.0, 15), (1.0, 15), (float("nan"), 15), (0.99, 0), (0.99, 1), (0.99, 40)])
def test_settings_at_their_limits(min_score, min_overlap):
    """min_score < 0: the first offset is taken whatever it scores; 0: any overlap with a counted position; >= 1 or NaN: none.  min_overlap 0
    starts at p = len1, where overlap_score returns 0."""
    seq, qual, pairs, _ = _srself.make_batch(20, 16, 60, seed=9)
    r = host.sr_merge_self_overlaps(seq, qual, pairs, min_score=min_score, min_overlap=min_overlap)
    first = np.where(pairs["len1"] > min_overlap, pairs["len1"].astype(np.int64) - min_overlap, -1)
    if min_score < 0:
        assert np.array_equal(r.overlap_pos, np.where(first > 0, first, -1))
    elif min_score == 0:
        assert np.array_equal(r.overlap_pos, np.where(first > 0, np.minimum(first, pairs["len1"].astype(np.int64) - 1), -1))
    elif not min_score < 1:
        assert (r.overlap_pos == -1).all()
    else:
        assert ((r.overlap_pos == -1) | (r.overlap_pos <= first)).all()
    t = host.sr_merge_self_overlaps(seq, qual, pairs, min_score=min_score, min_overlap=min_overlap, n_threads=7)
    _srself.assert_same(t, r, "threads")
