"""What the threshold tests of test_gpu_threshold_band.py rest on, checked without a GPU: the anchors exist, a threshold walked over an
anchor's score crosses the whole guard band, the oracle's class flips exactly where `score > T` does, and hc_finalize_batch — a pure host
function, the half that decides what the device hands over as HC_CLS_AMBIG — agrees with the oracle at every one of those thresholds."""
import ctypes as C

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd.records import RESULT_DTYPE
from tests import _band as B

KINDS = {"paired": ["min-sub", "max-sub", "min-sub", "max-sub", "twin", "exact", "mc"], "single": ["single"]}


@pytest.fixture(scope="module", params=[None, 6, 40, 60, 70], ids=lambda n: f"{n or 'hq'}_quals")
def batches(oracle, request):
    return B.anchors(oracle, request.param)


def finalize_all_ambiguous(ref, st):
    """hc_finalize_batch on the oracle's (x1, x2, mm, n) with every record's class forced to HC_CLS_AMBIG: the host decides everything."""
    res = np.zeros(ref.size, dtype=RESULT_DTYPE)
    res["x1"], res["x2"], res["mm"] = ref["x1"], ref["x2"], ref["mm"]
    res["n_cls"] = ref["n"] | (np.uint32(4) << 28)
    cs = st.to_c()
    score, mrate, cls = np.empty(ref.size), np.empty(ref.size), np.empty(ref.size, np.uint32)
    assert N.lib.hc_finalize_batch(C.byref(cs), res.ctypes.data, ref.size, score.ctypes.data, mrate.ctypes.data, cls.ctypes.data) == 0
    return score, mrate, cls


def check_host(oracle, batch, st):
    ref = oracle.score_batch(batch.reads, st, batch.cand)
    assert (ref["status"] == 0).all()
    score, mrate, cls = finalize_all_ambiguous(ref, st)
    assert np.array_equal(cls, ref["cls"]), st
    assert np.array_equal(score.view(np.uint64), ref["score"].view(np.uint64)), st
    assert np.array_equal(mrate.view(np.uint64), ref["mismatch_rate"].view(np.uint64)), st
    return ref


def test_every_anchor_exists(batches):
    for key, kinds in KINDS.items():
        assert [a.kind for a in batches[key].anchors] == kinds, (key, batches[key].anchors)
        assert batches[key].cand.size <= 512
    p = batches["paired"]
    by = {a.name: a for a in p.anchors}
    assert p.cand["ord"][by["min-sub-ord1"].index] == ord("1") and p.cand["ord"][by["min-sub-ord2"].index] == ord("2")
    i = by["min-sub-ord1"].index
    assert p.cand["ori1"][i] == 0 or p.cand["ori2"][i] == 0, "one paired anchor is meant to have a reverse-complemented partner"
    assert {by["min-sub-ord1"].which, by["min-sub-ord2"].which} == {"x1", "x2"}
    k_hi, k_lo = B.edge_hits(*B.anchor_xs(p, by["exact"]))
    assert k_hi is not None and k_lo is not None and k_hi < -1 and k_lo > 0, "the exact anchor is meant to BE each end of the band once"
    t = by["twin"].index
    assert p.ref["x1"][t].view(np.uint64) == p.ref["x2"][t].view(np.uint64) and p.ref["mm"][t] > 0


def test_the_band_model_at_the_ends_of_the_scale():
    inf = float("inf")
    assert B.band(float("nan")) == (inf, inf) and B.band(1.0) == (inf, inf) and B.band(1.5) == (inf, inf)
    assert B.band(-1e-300) == (-inf, -inf) and B.band(0.0) == B.band(-0.0) == (-760.0, -740.0)
    lo, hi = B.band(0.97)
    assert lo < np.log(0.97) < hi and hi - lo == 2.0 ** -48
    lo, hi = B.band(1e-3)
    assert abs((hi - lo) / (2.0 ** -48 * abs(np.log(1e-3))) - 1) < 0.05   # the band widens with |ln T| (lo and hi are rounded to ulp(ln T) = 2^-50 here)
    # the three-valued rule on hand-made records: x1, x2, mm, n
    import haploconduct_amd as hc
    st = hc.Settings(edge_threshold=0.9, ov_threshold=0.5)
    le, lo_ = np.log(0.9), np.log(0.5)
    x1 = np.array([le, le, le, -0.01, lo_, lo_, -5.0, le, -inf])
    x2 = np.array([np.nan, -0.01, -5.0, -0.01, np.nan, -0.01, lo_, le, np.nan])
    mm = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1])
    assert B.model_class(x1, x2, mm, np.full(9, 100), st).tolist() == [4, 4, 0, 2, 4, 4, 0, 4, 0]
    assert B.model_class(x1, x2, np.zeros(9, int), np.full(9, 100), st).tolist() == [4, 4, 3, 2, 3, 3, 3, 4, 3]
    assert B.model_class(x1, x2, mm, np.full(9, 100), hc.Settings(edge_threshold=-1.0, ov_threshold=-1.0)).tolist() == [2] * 9


def test_edge_sweeps_cross_the_band_and_flip_once(oracle, batches):
    for key in ("paired", "single"):
        batch = batches[key]
        for a in batch.anchors:
            if a.kind == "mc":
                continue
            sw = B.edge_sweep(batch, a)
            regions = [r for _, _, r in sw]
            assert {"below", "band", "above"} == set(regions), (a, regions)
            ks = [k for k, _, _ in sw]
            assert ks == list(range(ks[0], ks[-1] + 1)) and ks[0] <= -B.OUTSIDE and ks[-1] >= B.OUTSIDE - 1
            # x above the band at the low end, below it at the high end, one run of "band" in between, k = -1 and 0 inside it
            first, last = regions.index("band"), len(regions) - 1 - regions[::-1].index("band")
            assert set(regions[:first]) == {"above"} and set(regions[last + 1:]) == {"below"} and set(regions[first:last + 1]) == {"band"}
            assert ks[first] <= -1 and ks[last] >= 0
            cls = [int(check_host(oracle, batch, st)["cls"][a.index]) for _, st, _ in sw]
            if a.flips:
                assert all(c == 2 for k, c in zip(ks, cls) if k <= -1) and all(c == 1 for k, c in zip(ks, cls) if k >= 0), (a, list(zip(ks, cls)))
            else:
                assert set(cls) == {1}, (a, list(zip(ks, cls)))


@pytest.mark.parametrize("with_mc", [False, True])
def test_ov_sweeps_cross_the_band_and_flip_once(oracle, batches, with_mc):
    for key, name in (("paired", "min-sub-ord1"), ("paired", "min-sub-ord2"), ("single", "single")):
        batch = batches[key]
        a = {a.name: a for a in batch.anchors}[name]
        sw = B.ov_sweep(batch, a, B.rate(batch, a) if with_mc else 0.0)
        assert {"below", "band", "above"} == {r for _, _, r in sw}
        for k, st, _ in sw:
            ref = check_host(oracle, batch, st)
            assert int(ref["cls"][a.index]) == (3 if with_mc else (1 if k <= -1 else 0)), (a, k)
            assert not (ref["cls"] == 2).any()
        if with_mc:
            assert (ref["cls"] == 3).any() and (ref["cls"] != 3).any()


def test_merge_contigs_at_the_mismatch_rate(oracle, batches):
    batch = batches["paired"]
    a = {a.name: a for a in batch.anchors}["mc"]
    for tag, st, yes in B.mc_settings(batch, a):
        ref = check_host(oracle, batch, st)
        assert (int(ref["cls"][a.index]) == 3) == yes, tag


def test_thresholds_at_the_ends_of_the_scale(oracle, batches):
    for key in ("paired", "single"):
        for st in B.special_settings():
            check_host(oracle, batches[key], st)
