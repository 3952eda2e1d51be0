"""Shared by the self-overlap tests (hc_sr_merge_self_overlaps, include/hcsr.h): the golden file's cases as calls, the synthetic
batches, and the comparison of two results."""
import json
import os

import numpy as np

from haploconduct_amd import consensus as SR
from haploconduct_amd import synth
from haploconduct_amd.records import Settings

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "self_overlap.json")


def check_against_golden(run):
    """run(seq, qual, pairs, settings: Settings, min_qual) -> SrSelfResult.  The cases are grouped by their settings: one call per group."""
    g = json.load(open(GOLDEN))
    assert "probe with substitutes" in g["provenance"] and g["min_score"] == 0.99 and g["min_overlap"] == 15
    groups = {}
    for c in g["cases"]:
        groups.setdefault((c["mismatch"], c["min_read_len"], c["min_qual"]), []).append(c)
    n = 0
    for (mm, mrl, mq), cases in sorted(groups.items()):
        seq, qual, pairs = SR.pack_pairs([(c["seq1"].encode(), c["qual1"].encode(), c["seq2"].encode(), c["qual2"].encode()) for c in cases])
        r = run(seq, qual, pairs, Settings(mismatch=mm, min_read_len=mrl), mq)
        for i, c in enumerate(cases):
            s, q = r.merged(i)
            assert int(r.status[i]) == (SR.SR_SELF_MERGED if c["merged"] else SR.SR_SELF_NONE), c["name"]
            assert int(r.overlap_pos[i]) == c["overlap_pos"], (c["name"], int(r.overlap_pos[i]), c["overlap_pos"])
            assert s.decode() == c["merged_seq"] and q.decode() == c["merged_qual"], c["name"]
            assert (r.score[i] > 0.99) == bool(c["merged"]), c["name"]
            n += 1
    return n


def quality_alphabet(name="savage_singles"):
    h = json.load(open(os.path.join(HERE, "golden", "quality_histograms.json")))[name]["counts"]
    vals = np.array(sorted(int(k) for k in h), np.uint8)
    w = np.array([h[str(int(v))] for v in vals], np.float64)
    return vals, w / w.sum()


def make_batch(n_pairs, lo, hi, seed, qvals=None, qweights=None, **kw):
    """synth.make_mate_pairs with the quality alphabet of the SAVAGE example reads where none is given."""
    if qvals is None:
        qvals, qweights = quality_alphabet()
    return synth.make_mate_pairs(n_pairs, lo, hi, seed, qvals=qvals, qweights=qweights, **kw)


def band_batch(log2_width, seed=78):
    """A batch whose deciding offsets crowd around min_score = 0.99, for the guard band of relative width 2^log2_width, and the mask of the
    pairs in which a scan has to CONTINUE below an offset of the band: (seq, qual, pairs, rejected_in_band).
    400 pairs without substitutions whose qualities are Q20 (45 %) or Q30: a term is log p = -0.0020 (Q30, Q30), -0.0111 (Q30, Q20) or -0.0201
    (Q20, Q20), their mean -0.0101, and ln 0.99 = -0.01005, so the true overlaps score on both sides of 0.99 and close to it.  Eight more
    pairs are built to merge BELOW a rejected offset: mate 1 = 30 random bases + R (40 bases) + R[:20], mate 2 = R, everything Q30 but 18 of
    mate 1's last 20 bases at Q20.  At p = 70 the 20 positions give x = (2 * -0.0020 + 18 * -0.0111) / 20 = -0.0101: below ln 0.99 and, for
    widths down to 2^-10 (lower edge -0.01103), inside the band; at p = 30 all 40 positions are (Q30, Q30): 0.998.
    The mask comes from the mirror alone: with min_score a little above the band's lower edge it stops at the first offset the device must
    report as a hit or as in the band, or above it; where that offset scores <= 0.99 and the mirror's answer for 0.99 lies below it, the
    device call's host share has rejected an offset and gone on."""
    import math
    from haploconduct_amd import host
    rng = np.random.default_rng(seed)
    seq, qual, pairs, _ = make_batch(400, 16, 300, seed=seed, max_overlap=60, sub_rate=0.0, qvals=np.array([53, 63], np.uint8), qweights=np.array([0.45, 0.55]))
    built = []
    for _ in range(8):
        x, r = (bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in (30, 40))
        q1 = np.full(90, 63, np.uint8)
        q1[70 + rng.permutation(20)[:18]] = 53
        built.append((x + r + r[:20], q1.tobytes(), r, bytes([63]) * 40))
    s2, q2, p2 = SR.pack_pairs(built)
    p2["off1"] += seq.size
    p2["off2"] += seq.size
    seq, qual, pairs = np.concatenate([seq, s2]), np.concatenate([qual, q2]), np.concatenate([pairs, p2])
    lt = math.log(0.99)
    lower_edge = lt - 2.0 ** log2_width * max(1.0, abs(lt))  # make_band, hc_api.cpp
    first = host.sr_merge_self_overlaps(seq, qual, pairs, min_score=math.exp(lower_edge) * (1 + 2.0 ** -20), n_threads=16)
    ref = host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16)
    return seq, qual, pairs, (first.overlap_pos > ref.overlap_pos) & (first.score <= 0.99)


def assert_same(dev, ref, what=""):
    assert np.array_equal(dev.status, ref.status), f"{what}: statuses differ at {np.flatnonzero(dev.status != ref.status)[:5]}"
    assert np.array_equal(dev.overlap_pos, ref.overlap_pos), f"{what}: offsets differ at {np.flatnonzero(dev.overlap_pos != ref.overlap_pos)[:5]}"
    assert np.array_equal(dev.score.view(np.uint64), ref.score.view(np.uint64)), f"{what}: scores differ in their bits"
    assert np.array_equal(dev.out_off, ref.out_off), f"{what}: output offsets differ"
    assert np.array_equal(dev.merged_seq, ref.merged_seq), f"{what}: merged bases differ"
    assert np.array_equal(dev.merged_qual, ref.merged_qual), f"{what}: merged qualities differ"
    assert dev.n_merged == ref.n_merged and dev.n_offsets == ref.n_offsets
