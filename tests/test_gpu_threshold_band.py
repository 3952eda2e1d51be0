"""The admission class AT the thresholds.  The scoring kernel decides `score > T` in x-space against a guard band around ln T; a record
inside the band is HC_CLS_AMBIG and the host decides it, everything else is final on the device (a DROP never reaches the host, a NONEDGE
is written without hc_finalize).  Here a threshold is set to an anchor's own oracle score moved ulp by ulp (tests/_band.py), so that the
anchor crosses the band's two edges and `score == T`, and every record of the batch is held to

  band identity  hc_get_info's band is _band.band(T), bit for bit;
  soundness      the device class is the oracle's or AMBIG, the finalised class, score and mismatch rate are the oracle's;
  tightness      the device class is _band.model_class(...): AMBIG where, and only where, an x lies in a band that still matters;
  liveness       over a sweep the anchor is AMBIG in every "band" setting and decided in every other one.

tests/test_threshold_anchors_host.py checks, without a GPU, that the sweeps do cross the band and that the oracle flips between k = -1 and 0."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import host, synth
from haploconduct_amd.records import REC_FULL, result_cls, result_n
from tests import _band as B

pytestmark = pytest.mark.gpu

_cache = {}
SEEN = {"records": 0, "ambig": 0}   # device records checked so far, and how many of them were HC_CLS_AMBIG (printed; pytest -rA shows it)


def batches(oracle, n_quals=None):
    if n_quals not in _cache:
        b = B.anchors(oracle, n_quals)
        for batch in b.values():
            for a in (batch.cand, batch.ref):
                a.flags.writeable = False
        _cache[n_quals] = b
    return _cache[n_quals]


def anchor(batch, name):
    return {a.name: a for a in batch.anchors}[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_entry(sc, cand):
    return sc.score_batch(cand)


def device_compact_entry(sc, cand):
    """Compact records on the context's own device entry point: the one the locality launch serves."""
    import torch

    cd = sc.pack_cands(cand)
    d_in = torch.from_numpy(cd.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((cd.size * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    sc.score_cands_device(d_in.data_ptr(), cd.size, d_out.data_ptr())
    sc.synchronize()
    return d_out.cpu().numpy().view(hc.RESULT_DTYPE)


def check(oracle, sc, batch, st, entry=host_entry, expect_kernel=None):
    """One setting, the whole batch: band identity, soundness, tightness.  Returns (oracle records, device classes)."""
    sc.reset(st)
    sc.set_reads(batch.reads)
    if expect_kernel:
        expect_kernel(sc.kernel_info(batch.cand.size))
    info = sc.info()
    for key, T in (("x_edge", st.edge_threshold), ("x_ov", st.ov_threshold)):
        assert bits(info[key]).tolist() == bits(B.band(T)).tolist(), f"the library's band for T = {T!r} is {info[key]}, the model's {B.band(T)}"
    ref = oracle.score_batch(batch.reads, st, batch.cand)
    assert (ref["status"] == 0).all()
    res = entry(sc, batch.cand)
    score, mrate, cls = sc.finalize(res)
    one = ref["n_subs"] == 1
    assert np.array_equal(bits(res["x1"]), bits(ref["x1"])) and np.array_equal(bits(res["x2"])[~one], bits(ref["x2"])[~one])
    assert np.isnan(res["x2"][one]).all()
    assert np.array_equal(res["mm"], ref["mm"]) and np.array_equal(result_n(res), ref["n"])
    dev = result_cls(res)
    SEEN["records"] += dev.size
    SEEN["ambig"] += int((dev == 4).sum())
    assert ((dev == ref["cls"]) | (dev == 4)).all(), f"a class the device decided differs from the oracle's: {st}"
    assert np.array_equal(cls, ref["cls"]), f"finalised class differs: {st}"
    assert np.array_equal(bits(score), bits(ref["score"])) and np.array_equal(bits(mrate), bits(ref["mismatch_rate"]))
    want = B.model_class(ref["x1"], ref["x2"], ref["mm"], ref["n"], st)
    bad = np.nonzero(dev != want)[0]
    assert bad.size == 0, f"device class {dev[bad][:5]} where the three-valued rule says {want[bad][:5]} (records {bad[:5]}): {st}"
    return ref, dev


def check_sweep(oracle, sc, batch, a, sw, live, entry=host_entry, expect_kernel=None):
    """Every setting of a sweep; liveness of the anchor.  Returns the number of AMBIG records seen."""
    seen, n_ambig = set(), 0
    for k, st, region in sw:
        ref, dev = check(oracle, sc, batch, st, entry, expect_kernel)
        n_ambig += int((dev == 4).sum())
        d = int(dev[a.index])
        if live:
            assert (d == 4) == (region == "band"), f"{a.name}, k = {k} ({region}): device class {d}"
            seen.add(region)
        elif a.kind == "max-sub":
            assert d == int(ref["cls"][a.index]) != 4, f"{a.name}, k = {k}: the other sub-overlap decides, the device said {d}"
    if live:
        assert seen == {"below", "band", "above"}
    print(f"{a.name}: {len(sw)} settings, {n_ambig} AMBIG records; so far {SEEN['ambig']} of {SEEN['records']} device records were AMBIG")
    return n_ambig


EDGE_ANCHORS = [("paired", "min-sub-ord1"), ("paired", "max-sub-ord1"), ("paired", "min-sub-ord2"), ("paired", "max-sub-ord2"), ("paired", "twin"),
                ("paired", "exact"), ("single", "single")]


@pytest.mark.parametrize("key,name", EDGE_ANCHORS, ids=[n for _, n in EDGE_ANCHORS])
def test_edge_threshold_over_an_anchor(oracle, key, name):
    batch = batches(oracle)[key]
    a = anchor(batch, name)
    with hc.EdgeScorer(hc.Settings()) as sc:
        n = check_sweep(oracle, sc, batch, a, B.edge_sweep(batch, a), live=a.flips)
    assert n > 0 or not a.flips


@pytest.mark.parametrize("with_mc", [False, True], ids=["merge_contigs_0", "merge_contigs_at_the_anchors_rate"])
@pytest.mark.parametrize("key,name", [("paired", "min-sub-ord1"), ("paired", "min-sub-ord2"), ("single", "single")], ids=["ord1", "ord2", "single"])
def test_ov_threshold_over_an_anchor(oracle, key, name, with_mc):
    """Nothing is admitted by its score (edge threshold 1): NONEDGE against DROP, the `o == 2` path.  With merge_contigs at the anchor's own
    mismatch rate the anchor is EDGE_MC whatever its `o`: an ambiguous ov test that is not reached must not make the record AMBIG."""
    batch = batches(oracle)[key]
    a = anchor(batch, name)
    sw = B.ov_sweep(batch, a, B.rate(batch, a) if with_mc else 0.0)
    with hc.EdgeScorer(hc.Settings()) as sc:
        if not with_mc:
            check_sweep(oracle, sc, batch, a, sw, live=True)
        else:
            for k, st, region in sw:
                ref, dev = check(oracle, sc, batch, st)
                assert dev[a.index] == ref["cls"][a.index] == 3, (k, region)
                assert (ref["cls"] == 3).any() and (ref["cls"] != 3).any()


def test_merge_contigs_at_below_and_above_a_mismatch_rate(oracle):
    batch = batches(oracle)["paired"]
    a = anchor(batch, "mc")
    with hc.EdgeScorer(hc.Settings()) as sc:
        for tag, st, yes in B.mc_settings(batch, a):
            ref, dev = check(oracle, sc, batch, st)
            assert (ref["cls"][a.index] == 3) == yes and (dev[a.index] == 3) == yes, (tag, st.merge_contigs, dev[a.index])


def test_thresholds_at_the_ends_of_the_scale(oracle):
    with hc.EdgeScorer(hc.Settings()) as sc:
        for key in ("paired", "single"):
            for st in B.special_settings():
                check(oracle, sc, batches(oracle)[key], st)


# -- every form the class is computed in ---------------------------------------------------------------------------------------

FORMS = {
    "per_lane_4": ({"HC_FETCH_GROUP": "4"}, "paired"),
    "per_lane_2": ({"HC_FETCH_GROUP": "2"}, "paired"),
    "coop_registers": ({"HC_FETCH_GROUP": "coop"}, "paired"),
    "coop_lds_dma": ({"HC_FETCH_GROUP": "coop", "HC_COOP_DMA_MIN": "1"}, "paired"),
    "bucketed": ({"HC_BALANCE": "1"}, "single"),
    "locality_ticket": ({"HC_COOP_DMA_MIN": "1", "HC_LOCALITY": "1", "HC_LOCALITY_MIN": "1"}, "paired"),
}


def _expect_kernel(form, n_quals):
    def expect(info):
        head = info.split(" encoding=")[0]
        if form.startswith("per_lane"):
            want = "hc::score_kernel_wide_wg<uint8_t, " if n_quals in (40, 60) else "hc::score_kernel<"
            assert info.startswith(want), info
        elif form == "bucketed":
            assert "length-bucketed" in info and "score_kernel_coop<" in info, info
        else:
            assert "score_kernel_coop<" + ("uint16_t" if n_quals > 60 else "uint8_t") in info and "length-bucketed" not in info, info
            if n_quals <= 60:  # (16-bit symbols have no LDS-DMA form)
                assert (", 0, true>" in head) == (form != "coop_registers"), info
    return expect


@pytest.mark.parametrize("n_quals", [6, 40, 60, 70])
@pytest.mark.parametrize("form", list(FORMS))
def test_reduced_sweeps_through_every_kernel_form(oracle, monkeypatch, form, n_quals):
    """Far below, the last setting outside and the first inside each edge of the band, k = -1, 0, +1 and far above, through the per-lane
    kernels, the cooperative kernel in its register and LDS-DMA forms (which assembles its class parameters itself), the bucketed launch
    on the mixed-length singles and the locality / ticket form; 8-bit, wide-table and 16-bit symbols."""
    env, key = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    batch = batches(oracle, n_quals)[key]
    entry = device_compact_entry if form == "locality_ticket" else host_entry
    expect = _expect_kernel(form, n_quals)
    n_ambig = 0
    with hc.EdgeScorer(hc.Settings()) as sc:
        for a in batch.anchors:
            if a.kind in ("mc", "max-sub"):
                continue
            n_ambig += check_sweep(oracle, sc, batch, a, B.reduced(B.edge_sweep(batch, a)), live=True, entry=entry, expect_kernel=expect)
            if a.kind != "twin":
                n_ambig += check_sweep(oracle, sc, batch, a, B.reduced(B.ov_sweep(batch, a)), live=True, entry=entry, expect_kernel=expect)
        assert sc.info()["qual_alphabet"] == n_quals
        if form == "locality_ticket":
            assert sc.locality_order().size == batch.reads.n_reads
    assert n_ambig > 0


# -- what consumes the device class ------------------------------------------------------------------------------------------------

def _consumer_setting(oracle, k):
    """The ov threshold at (k = 0: the oracle drops the anchor) or one ulp under (k = -1: it keeps it) the anchor's score; the anchor is
    AMBIG on the device either way."""
    batch = batches(oracle)["paired"]
    a = anchor(batch, "min-sub-ord1")
    st = {kk: s for kk, s, _ in B.ov_sweep(batch, a)}[k]
    return batch, a, st


@pytest.mark.parametrize("k", [0, -1])
def test_compaction_keeps_an_ambiguous_record(oracle, k):
    import torch

    batch, a, st = _consumer_setting(oracle, k)
    cand = batch.cand
    with hc.EdgeScorer(hc.Settings()) as sc:
        ref, dev = check(oracle, sc, batch, st)
        assert dev[a.index] == 4 and ref["cls"][a.index] == (0 if k == 0 else 1)
        full = sc.score_batch(cand)
        idx, res = sc.score_batch_compact(cand)
        d_in = torch.from_numpy(cand.view(np.uint8).reshape(-1).copy()).cuda()
        d_out = torch.empty(cand.size * 24, dtype=torch.uint8, device="cuda")
        d_idx = torch.zeros(cand.size, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        sc.score_batch_device(d_in.data_ptr(), cand.size, d_out.data_ptr())
        sc.compact_device(d_out.data_ptr(), cand.size, d_idx.data_ptr(), d_cnt.data_ptr())
        sc.synchronize()
        idx2 = d_idx[:int(d_cnt.item())].cpu().numpy().view(np.uint32)
        assert d_out.cpu().numpy().tobytes() == full.tobytes()
        kept_by_oracle = np.nonzero(ref["cls"] != 0)[0]
        for got in (idx, idx2):
            assert a.index in got, "compaction removed the ambiguous record"
            assert np.isin(kept_by_oracle, got).all(), "compaction removed a record the oracle keeps"
            extra = np.setdiff1d(got, kept_by_oracle)
            assert (dev[extra] == 4).all(), "compaction kept a record that is neither the oracle's nor ambiguous"
            assert np.array_equal(got, np.nonzero(dev != 0)[0])
        assert res.tobytes() == full[idx].tobytes()
        _, _, cls = sc.finalize(res)
        assert np.array_equal(idx[cls != 0], kept_by_oracle)


@pytest.mark.parametrize("k", [0, -1])
def test_row_sink_and_narrow_rows_carry_an_ambiguous_record(oracle, k):
    import torch

    batch, a, st = _consumer_setting(oracle, k)
    cand = batch.cand
    base = 1000
    with hc.EdgeScorer(hc.Settings()) as sc:
        ref, dev = check(oracle, sc, batch, st)
        full = sc.score_batch(cand)
        kept = np.nonzero(dev != 0)[0]
        assert dev[a.index] == 4
        want = np.zeros((kept.size, 4), np.int64)
        want[:, 0] = kept + base
        want[:, 1], want[:, 2] = full["x1"][kept].view(np.int64), full["x2"][kept].view(np.int64)
        want[:, 3] = full["mm"][kept].astype(np.int64) | (full["n_cls"][kept].astype(np.int64) << 32)
        d_in = torch.from_numpy(cand.view(np.uint8).reshape(-1).copy()).cuda()
        d_out = torch.empty(cand.size * 24, dtype=torch.uint8, device="cuda")
        cap = kept.size + 3
        payload = torch.full((cap + 1, 4), -1, dtype=torch.int64, device="cuda")
        sc.score_pack_device(d_in.data_ptr(), cand.size, d_out.data_ptr(), cap, base, payload.data_ptr(), None, REC_FULL)
        sc.synchronize()
        p = payload.cpu().numpy()
        assert int(p[0, 0]) == kept.size
        rows = p[1:1 + kept.size]
        assert np.array_equal(rows[np.argsort(rows[:, 0])], want)
        # the compacted records packed by hc_pack_rows_device: the same rows, in index order
        d_idx = torch.zeros(cand.size, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_rows = torch.full((cap, 4), -1, dtype=torch.int64, device="cuda")
        sc.compact_device(d_out.data_ptr(), cand.size, d_idx.data_ptr(), d_cnt.data_ptr())
        sc.pack_rows_device(d_out.data_ptr(), d_idx.data_ptr(), d_cnt.data_ptr(), cap, base, d_rows.data_ptr())
        sc.synchronize()
        assert int(d_cnt.item()) == kept.size and np.array_equal(d_rows.cpu().numpy()[:kept.size], want)
        # the 24-byte rows: x1, x2, index | mm << 32 | n << 46 | class << 60
        narrow = torch.full((cap + 1, 3), -1, dtype=torch.int64, device="cuda")
        sc.narrow_payload_device(payload.data_ptr(), cap, narrow.data_ptr())
        sc.synchronize()
        nw = narrow.cpu().numpy().view(np.uint64)
        assert nw[0].tolist() == [kept.size, 0, 0]
        nr = nw[1:1 + kept.size]
        nr = nr[np.argsort(nr[:, 2] & np.uint64(0xFFFFFFFF))]
        assert np.array_equal(nr[:, 0], want[:, 1].view(np.uint64)) and np.array_equal(nr[:, 1], want[:, 2].view(np.uint64))
        word = (kept + base).astype(np.uint64) | (full["mm"][kept].astype(np.uint64) << np.uint64(32)) | \
               (result_n(full)[kept].astype(np.uint64) << np.uint64(46)) | (dev[kept].astype(np.uint64) << np.uint64(60))
        assert np.array_equal(nr[:, 2], word)
        at = int(np.nonzero(kept == a.index)[0][0])
        assert int(nr[at, 2] >> np.uint64(60)) == 4 and int(want[at, 3] >> 60) == 4
        assert nr[at, 0] == bits(ref["x1"][a.index])[0] and nr[at, 1] == bits(ref["x2"][a.index])[0]


def _stage_settings(batch, k):
    """edge_threshold at the min-sub score of one line (moved by k ulps), ov_threshold at the score of another, low-scoring line: most
    lines survive, one line is AMBIG against each threshold."""
    a = anchor(batch, "min-sub-ord1")
    T = {kk: s.edge_threshold for kk, s, _ in B.edge_sweep(batch, a)}[k]
    score = np.minimum(batch.ref["ov1"], batch.ref["ov2"])
    order = np.argsort(score)
    low = next(int(i) for i in order[order.size // 10:] if i != a.index and score[i] > 0.01 and batch.ref["mm"][i] > 0)
    assert float(score[low]) < T
    return hc.Settings(edge_threshold=T, ov_threshold=float(score[low]), min_overlap_len=0, n_threads=4), a, low


@pytest.mark.parametrize("k", [0, -1])
def test_stage_with_a_line_at_each_threshold(oracle, tmp_path, k):
    from tests.test_gpu_stage import run_both

    batch = batches(oracle)["paired"]
    st, a, low = _stage_settings(batch, k)
    ref = oracle.score_batch(batch.reads, st, batch.cand)
    assert ref["cls"][a.index] == (1 if k == 0 else 2) and ref["cls"][low] == 0
    lines = synth.records_to_lines(batch.cand, batch.reads)
    edges, c = run_both(oracle, tmp_path, batch.reads, lines, st, f"band{k}")
    assert c["ambiguous"] >= 2, c
    print(f"stage, k = {k}: {c['ambiguous']} ambiguous rows finalised on the host")
    assert edges.size > 0 and c["nonedges_written"] > 0


def test_stage_whose_lines_mostly_survive_with_lines_at_the_thresholds(oracle, tmp_path, monkeypatch):
    """The same file sixty times over in one text block: more rows survive than the block's first row buffers hold, so the block grows them
    and runs its device half again, and the rows are finalised from the lines the device kept."""
    from tests.test_gpu_stage import FIELDS

    monkeypatch.setenv("HC_TEXT_BLOCK", str(1 << 20))
    batch = batches(oracle)["paired"]
    st, a, low = _stage_settings(batch, 0)
    lines = synth.records_to_lines(batch.cand, batch.reads) * 60
    ov = str(tmp_path / "overlaps.txt")
    open(ov, "w").write("\n".join(lines) + "\n")
    p1, p2 = str(tmp_path / "p1.fastq"), str(tmp_path / "p2.fastq")
    batch.reads.write_fastq(None, p1, p2)
    rc, g, oc = oracle.construct_edges(batch.reads, st, ov, str(tmp_path / "ref_nonedge.txt"))
    assert rc == 0
    out = tmp_path / "out"
    out.mkdir()
    with host.EdgeCalculatorStage(st, paired1=p1, paired2=p2, overlaps=ov, output_dir=str(out) + "/") as ec:
        ec.construct_edges()
        edges, inc, c = ec.edges(), ec.inclusions(), ec.counters()
    assert c["host_blocks"] == 0 and c["regrown_blocks"] >= 1, c
    assert c["ambiguous"] >= 2 * 60, c
    print(f"stage, sixty copies: {c['ambiguous']} ambiguous rows finalised on the host, {c['regrown_blocks']} block(s) regrown")
    want = g.all_edges()
    assert edges.size == want.size > 0
    for f in FIELDS:
        x, y = edges[f], want[f]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f
    assert np.array_equal(inc, g.inclusions())
    assert (out / "nonedge_overlaps.txt").read_bytes() == (tmp_path / "ref_nonedge.txt").read_bytes()
    for f in ("inclusion_count", "dup_count", "edges_added", "nonedges_written", "prefilter_rejected", "lines_read", "scored"):
        assert c[f] == getattr(oc, f), f
