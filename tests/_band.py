"""The admission class at its thresholds: a plain model of the guard band and the data that puts an x inside it.

The scoring kernel decides `score > T` in x-space (x = mean log-probability, score = exp(x)) against a band around ln T that the host
builds in make_band (hc_api.cpp); an x inside (lo, hi] is HC_CLS_AMBIG and the host's libm decides.  This module restates the band, picks
candidates ("anchors") whose oracle score becomes the threshold, walks the threshold ulp by ulp across the band, and restates the documented
three-valued rule.  The model is used for the TIGHTNESS of the device class only (AMBIG where, and only where, the rule says so); what is
right is always the oracle's word."""
import math
from collections import namedtuple

import numpy as np

import haploconduct_amd as hc
from haploconduct_amd import synth
from haploconduct_amd.records import OVERLAP_DTYPE

HQ = np.array([20, 30, 37, 37, 37, 40, 40, 40, 40], dtype=np.uint8) + 33
INF = float("inf")
CAP = 512          # |k| at which a sweep gives up
OUTSIDE = 8        # settings a sweep wants outside the band on each side


def band(T):
    """make_band's five cases: (lo, hi) of the x values the device leaves to the host for `exp(x) > T`."""
    if T != T:
        return INF, INF            # score > NaN: never
    if T < 0:
        return -INF, -INF          # every score passes
    if T == 0:
        return -760.0, -740.0      # exp(x) > 0 unless it underflows
    if T >= 1:
        return INF, INF            # x <= 0: never
    lt = math.log(T)
    d = math.ldexp(1.0, -49) * max(1.0, abs(lt))
    return lt - d, lt + d


def region(x, T):
    """Where x lies against the band of T: "above" (passes on the device), "below" (fails there) or "band" (the host decides)."""
    lo, hi = band(T)
    return "above" if x > hi else ("below" if x <= lo else "band")


def sweep(s, x):
    """[(k, T, region)] for T = s moved by k ulps, k = 0, +-1, +-2, ... outward until x has been outside the band for OUTSIDE consecutive
    settings on each side; sorted by k.  Fails if |k| = CAP does not get there."""
    out = []
    for step in (1, -1):
        T, k, run = (s, 0, 0) if step == 1 else (math.nextafter(s, -INF), -1, 0)
        while run < OUTSIDE:
            assert abs(k) <= CAP, f"x = {x!r} is still inside the band of {T!r}, {k} ulps from the score {s!r}"
            r = region(x, T)
            run = 0 if r == "band" else run + 1
            out.append((k, T, r))
            T, k = math.nextafter(T, INF if step == 1 else -INF), k + step
    return sorted(out)


def edge_hits(s, x):
    """(k at which x == hi, k at which x == lo) over the sweep of s, None where x never is that end of the band."""
    hi = [k for k, T, _ in sweep(s, x) if band(T)[1] == x]
    lo = [k for k, T, _ in sweep(s, x) if band(T)[0] == x]
    return (hi[0] if hi else None, lo[0] if lo else None)


def reduced(sw):
    """The settings of a sweep that can tell two kernels apart: far below and far above, the last setting outside and the first inside
    each edge of the band, and k = -1, 0, +1."""
    want = {sw[0][0], sw[-1][0], -1, 0, 1}
    for a, b in zip(sw[:-1], sw[1:]):
        if a[2] != b[2]:
            want |= {a[0], b[0]}
    return [t for t in sw if t[0] in want]


def _tri(x, T):
    """exp(x) > T on the device: 1 yes, 0 no, 2 undecided.  A threshold below zero means "always"; a missing x (NaN) does not vote."""
    x = np.asarray(x, np.float64)
    if T < 0:
        return np.ones(x.shape, np.uint32)
    lo, hi = band(T)
    t = np.where(x > hi, 1, np.where(x <= lo, 0, 2)).astype(np.uint32)
    return np.where(np.isnan(x), 1, t).astype(np.uint32)


def _both(a, b):
    return np.where((a == 0) | (b == 0), 0, np.where((a == 1) & (b == 1), 1, 2))


def model_class(x1, x2, mm, n, settings):
    """The documented rule for the device's class: each x against each band, 0 wins over 2 and 2 over 1 across the two sub-overlaps,
    then EDGE, EDGE_MC, NONEDGE, DROP in that order, an undecided test that is reached giving AMBIG."""
    e = _both(_tri(x1, settings.edge_threshold), _tri(x2, settings.edge_threshold))
    o = _both(_tri(x1, settings.ov_threshold), _tri(x2, settings.ov_threshold))
    mc = np.asarray(mm).astype(np.float32).astype(np.float64) / np.asarray(n, np.float64) <= settings.merge_contigs
    low = np.where(mc, 3, np.where(o == 1, 1, np.where(o == 2, 4, 0)))
    return np.where(e == 1, 2, np.where(e == 2, 4, low)).astype(np.uint32)


Anchor = namedtuple("Anchor", "name kind index which flips")
Batch = namedtuple("Batch", "reads cand ref anchors")


def alphabet(n_quals=None, seed=0):
    """n_quals distinct quality bytes, drawn with a seed (None: the HQ set of the parity tests, four values weighted towards the high ones)."""
    if n_quals is None:
        return HQ
    return np.random.default_rng(1000 + n_quals + seed).choice(np.arange(33, 127), size=n_quals, replace=False).astype(np.uint8)


def _twins(rng, quals, L=150):
    """Two pairs whose mates are identical; the second pair is the first one shifted by `p` with two substitutions inside the overlap.
    Scored forward at pos1 == pos2 == p with ord '1', both sub-overlaps read the same bytes: x1 == x2 bit for bit."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    p = 23
    a = acgt[rng.integers(0, 4, L)]
    b = np.concatenate([a[p:], acgt[rng.integers(0, 4, p)]])
    for at in (40, 90):
        b[at] = acgt[(int(np.searchsorted(acgt, b[at])) + 1) % 4]
    qa, qb = quals[rng.integers(0, quals.size, L)], quals[rng.integers(0, quals.size, L)]
    return [((a.tobytes(), qa.tobytes()),) * 2, ((b.tobytes(), qb.tobytes()),) * 2], p


def _score(ref, i, which):
    return float(ref["ov1" if which == "x1" else "ov2"][i])


def _alone(ref, i, which):
    """No other sub-overlap of the batch has the anchor's score: the anchor is alone at its threshold (a twin's own mate excepted)."""
    s = _score(ref, i, which)
    same = (ref["ov1"] == s).astype(int) + ((ref["ov2"] == s) & (ref["n_subs"] == 2)).astype(int)
    same[i] = 0
    return not same.any()


def anchors(oracle, n_quals=None, seed=21):
    """{"paired": Batch, "single": Batch}: two small seeded read sets with at most 512 candidates each, the oracle's records for them
    (x, ov, mm and n do not depend on the thresholds) and the named anchors of each."""
    quals = alphabet(n_quals)
    neutral = hc.Settings(edge_threshold=0.5, ov_threshold=0.25)
    # -- pairs of 2 x 150, three in ten stored reverse-complemented, plus the twins
    base, meta = synth.make_paired_dataset(150, 1500, flip_frac=0.3, seed=seed, quals=quals)
    pairs = [(base.seq(2 * r), base.seq(2 * r + 1)) for r in range(base.n_reads)]
    rng = np.random.default_rng(seed + 1)
    tw, p = _twins(rng, quals)
    reads = hc.ReadSet.from_lists((), pairs + tw)
    cand = synth.paired_candidates(meta, n_candidates=None, seed=seed + 1)
    cand = cand[np.sort(rng.choice(cand.size, min(cand.size, 511), replace=False))]
    twin = np.zeros(1, OVERLAP_DTYPE)
    twin["read1"], twin["read2"], twin["pos1"], twin["pos2"] = base.n_reads, base.n_reads + 1, p, p
    twin["ori1"], twin["ori2"], twin["ord"], twin["flags"] = 1, 1, ord("1"), 3
    twin["len1"], twin["len2"], twin["perc"] = 150 - p, 150 - p, 84
    cand = np.concatenate([cand, twin])
    ref = oracle.score_batch(reads, neutral, cand)
    assert (ref["status"] == 0).all()
    lo, hi = np.minimum(ref["ov1"], ref["ov2"]), np.maximum(ref["ov1"], ref["ov2"])
    ok = (ref["n_subs"] == 2) & (ref["mm"] > 0) & (lo > 0.01) & (hi < 0.9999) & (hi > lo * 1.001)
    ok[-1] = False
    found = []
    rc = (cand["ori1"] == 0) | (cand["ori2"] == 0)
    # one candidate per ord; the ord '1' one with a reverse-complemented partner and x1 the smaller, the ord '2' one with x2 the smaller
    for tag, want in (("ord1", ok & (cand["ord"] == ord("1")) & rc & (ref["ov1"] < ref["ov2"])),
                      ("ord2", ok & (cand["ord"] == ord("2")) & (ref["ov2"] < ref["ov1"]))):
        for i in np.nonzero(want)[0]:
            small, large = ("x1", "x2") if ref["ov1"][i] < ref["ov2"][i] else ("x2", "x1")
            if _alone(ref, i, small) and _alone(ref, i, large):
                found.append(Anchor("min-sub-" + tag, "min-sub", int(i), small, True))
                found.append(Anchor("max-sub-" + tag, "max-sub", int(i), large, False))
                break
    t = cand.size - 1
    if ref["mm"][t] > 0 and 0.01 < ref["ov1"][t] < 0.9999 and _alone(ref, t, "x1"):
        found.append(Anchor("twin", "twin", t, "x1", True))
    used = {a.index for a in found}
    # a candidate whose smaller x IS the upper end of the band at one setting of its sweep and the lower end at another: `>` against `>=`
    for i in np.nonzero(ok)[0]:
        small = "x1" if ref["ov1"][i] < ref["ov2"][i] else "x2"
        if int(i) not in used and _alone(ref, i, small) and None not in edge_hits(_score(ref, i, small), float(ref[small][i])):
            found.append(Anchor("exact", "exact", int(i), small, True))
            used.add(int(i))
            break
    for i in np.nonzero(ok)[0]:
        if int(i) not in used:
            found.append(Anchor("mc", "mc", int(i), "x1", False))
            break
    paired = Batch(reads, cand, ref, found)
    # -- single-end reads of mixed length (150 .. 600), four in ten stored reverse-complemented
    sreads, smeta = synth.make_single_dataset(120, 1500, len_lo=150, len_hi=600, flip_frac=0.4, seed=seed + 2, quals=quals, log_uniform=True)
    scand = synth.single_candidates(smeta, min_overlap=60, n_candidates=512, seed=seed + 3)
    sref = oracle.score_batch(sreads, neutral, scand)
    assert (sref["status"] == 0).all()
    sfound = []
    for i in np.nonzero((sref["mm"] > 0) & (sref["ov1"] > 0.01) & (sref["ov1"] < 0.9999))[0]:
        if _alone(sref, i, "x1"):
            sfound.append(Anchor("single", "single", int(i), "x1", True))
            break
    return {"paired": paired, "single": Batch(sreads, scand, sref, sfound)}


def anchor_xs(batch, a):
    """(score, x) of the sub-overlap an anchor stands on."""
    return _score(batch.ref, a.index, a.which), float(batch.ref[a.which][a.index])


def edge_sweep(batch, a):
    """[(k, settings, region)]: the edge threshold walked over the anchor's score, the ov threshold well below it."""
    s, x = anchor_xs(batch, a)
    return [(k, hc.Settings(edge_threshold=T, ov_threshold=0.5 * s), r) for k, T, r in sweep(s, x)]


def ov_sweep(batch, a, merge_contigs=0.0):
    """The ov threshold walked over the anchor's score with nothing admitted by its score (edge threshold 1): NONEDGE against DROP."""
    s, x = anchor_xs(batch, a)
    return [(k, hc.Settings(edge_threshold=1.0, ov_threshold=T, merge_contigs=merge_contigs), r) for k, T, r in sweep(s, x)]


def rate(batch, a):
    """The anchor's mismatch rate as the reference computes it: float(mismatch_count) / total_len."""
    return float(np.float32(batch.ref["mm"][a.index])) / float(batch.ref["n"][a.index])


def mc_settings(batch, a):
    """merge_contigs at the anchor's mismatch rate (admitted: <=), one ulp below it (not admitted) and one ulp above (admitted)."""
    r = rate(batch, a)
    return [(tag, hc.Settings(edge_threshold=1.0, ov_threshold=0.25, merge_contigs=v), yes)
            for tag, v, yes in (("at", r, True), ("below", math.nextafter(r, 0.0), False), ("above", math.nextafter(r, 1.0), True))]


def special_settings():
    """Thresholds at the ends of the scale.  (Left out: thresholds whose ln lies below every reachable x — x >= about -25 by the quality
    table — and subnormal ones; nothing can sit at them.)"""
    vals = [math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 0.0, -0.0, -0.5, float("nan")]
    out = [hc.Settings(edge_threshold=v, ov_threshold=0.5) for v in vals]
    out += [hc.Settings(edge_threshold=0.97, ov_threshold=v) for v in vals]
    out += [hc.Settings(edge_threshold=v, ov_threshold=v, merge_contigs=0.01) for v in vals]
    out += [hc.Settings(edge_threshold=0.9, ov_threshold=0.95), hc.Settings(edge_threshold=0.9, ov_threshold=0.95, merge_contigs=0.01),
            hc.Settings(edge_threshold=0.5, ov_threshold=1.0), hc.Settings(edge_threshold=-1.0, ov_threshold=0.97)]
    return out
