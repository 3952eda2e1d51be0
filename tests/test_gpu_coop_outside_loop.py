"""The cooperative scoring kernel outside its position loop (hc_kernels.hip: score_kernel_coop — candidate set-up, the pass prologue,
finish_sub, the result exchange, classify_and_store; hc_resolve.h: resolve_regular32): every form of the kernel against the oracle, bit
for bit on x1, x2, mm, n and class.

One regular store (16 singles + 48 pairs, all 150 bp) with 6 / 35 / 70 quality values (the packed, the wide and the 16-bit encoding) and
about 4 000 compact candidates whose count is no multiple of 64: every window length 1..150 on both positions, all orientations and
order codes, s-s / s-p / p-s / p-p mixed inside every wave (lanes that enter the second pass with L = 0), skip records, ids out of
range, read1 == read2, an invalid order code, pos >= length.  One read holds an N and one an invalid symbol inside a window, so the
re-scan (score_sub_slow) runs: an invalid QUALITY byte keeps the store regular (resolve_regular32), an invalid BASE makes it irregular
(resolve with descriptor look-ups) — both are run.  Each set goes through the register-staged form, the LDS-DMA form (HC_COOP_DMA_MIN),
a row-sink launch, and settings with merge_contigs > 0 and negative thresholds (the division arms and the *_all flags).  A set of 40
singles of 150..1 200 bp goes through the bucketed launch."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd.records import OVERLAP_DTYPE, REC_COMPACT, result_cls, result_n

pytestmark = pytest.mark.gpu

SKIP_BIT = np.uint32(0x80000000)  # include/hcedge.h: HC_CAND_SKIP
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
L = 150
N_SINGLE, N_PAIR = 16, 48
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _reads(n_quals, invalid):
    """invalid: 'qual' (a quality byte below 33: the store stays regular), 'base' (a base outside ACGTN: descriptor look-ups)."""
    rng = np.random.default_rng(1000 + n_quals)
    genome = ACGT[rng.integers(0, 4, 1200)]
    alphabet = (33 + np.arange(2, 2 + n_quals)).astype(np.uint8)

    def piece(s):
        seg = genome[s:s + L].copy()
        k = rng.random(L) < 0.01
        seg[k] = ACGT[rng.integers(0, 4, int(k.sum()))]
        return bytearray(seg.tobytes()), bytearray(alphabet[rng.integers(0, n_quals, L)].tobytes())

    singles = [piece(int(rng.integers(0, 1000))) for _ in range(N_SINGLE)]
    pairs = []
    for _ in range(N_PAIR):
        s = int(rng.integers(0, 600))
        pairs.append((piece(s), piece(s + int(rng.integers(200, 400)))))
    singles[3][0][70] = ord("N")       # an N inside a window: adds 0.0, counted as skipped
    pairs[5][0][0][40] = ord("N")
    if invalid == "base":
        singles[7][0][90] = ord("X")   # NaN row of the table -> the exact re-scan -> an error
        pairs[9][1][0][20] = ord("X")
    else:
        singles[7][1][90] = 20         # a quality byte outside [33, 127]
        pairs[9][1][1][20] = 20
    fix = lambda p: (bytes(p[0]), bytes(p[1]))
    return hc.ReadSet.from_lists([fix(p) for p in singles], [(fix(a), fix(b)) for a, b in pairs])


def _candidates(n_reads, n=4001, max_pos=L, seed=3):
    rng = np.random.default_rng(seed)
    assert n % 64 != 0
    c = np.zeros(n, OVERLAP_DTYPE)
    a = rng.integers(0, n_reads, n)
    c["read1"], c["read2"] = a, (a + 1 + rng.integers(0, n_reads - 1, n)) % n_reads  # singles and pairs mixed inside every wave
    # reads 7 (a single) and 16 + 9 (a pair) hold the invalid symbols, 3 and 16 + 5 the Ns: make sure they are scored often
    hot = rng.random(n) < 0.15
    c["read1"][hot] = rng.choice([3, 7, N_SINGLE + 5, N_SINGLE + 9], int(hot.sum()))
    c["read2"][hot & (c["read2"] == c["read1"])] = 0
    # every window length 1 .. max_pos on both positions (L - pos), the chunk / row / step boundaries among them, and pos >= length
    c["pos1"] = np.arange(n) % (max_pos + 3)
    c["pos2"] = (np.arange(n) * 7 + 5) % (max_pos + 3)
    c["ori1"], c["ori2"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
    c["ord"] = np.frombuffer(b"12", np.uint8)[rng.integers(0, 2, n)]
    c["ord"][rng.random(n) < 0.03] = ord("x")          # an invalid order code: malformed on a p-p record only
    c["len1"], c["len2"], c["perc"] = L, L, 50
    k = np.nonzero(rng.random(n) < 0.02)[0]
    c["read1"][k] = n_reads + rng.integers(0, 5, k.size)  # ids out of range
    k = np.nonzero(rng.random(n) < 0.02)[0]
    c["read2"][k] = 0xFFFFFFF0
    k = np.nonzero(rng.random(n) < 0.02)[0]
    c["read2"][k] = c["read1"][k]                      # read1 == read2
    skip = rng.random(n) < 0.05                        # interleaved skip records
    skip[[0, 63, 64, 65, n - 1]] = [True, False, True, True, True]
    return c, skip


def _compact(sc, cand, skip):
    cd = sc.pack_cands(cand)
    cd["pos2_bits"][skip] |= SKIP_BIT
    return cd


def _check(ref, res, cls, skip, where):
    ok = (ref["status"] == 0) & ~skip
    bad = (ref["status"] != 0) & ~skip
    dev = result_cls(res)
    n, mm = result_n(res), res["mm"]
    assert ok.sum() > 0.7 * ok.size and bad.sum() > 50 and skip.sum() > 50, where
    assert np.array_equal(_bits(res["x1"])[ok], _bits(ref["x1"])[ok]), where + ": x1"
    nan2 = np.isnan(ref["x2"])
    assert np.array_equal(np.isnan(res["x2"])[ok], nan2[ok]), where + ": x2 (which are NaN)"
    assert np.array_equal(_bits(res["x2"])[ok & ~nan2], _bits(ref["x2"])[ok & ~nan2]), where + ": x2"
    assert np.array_equal(mm[ok], ref["mm"][ok]) and np.array_equal(n[ok], ref["n"][ok]), where + ": mm / n"
    assert np.array_equal(cls[ok], ref["cls"][ok]), where + ": class (host-finalised)"
    assert ((dev[ok] == ref["cls"][ok]) | (dev[ok] == 4)).all(), where + ": class (device)"
    assert (dev[bad] == 7).all(), where + ": a malformed record or an invalid symbol is an error"
    for m, c in ((skip, 0), (bad & (ref["status"] <= -10), 7)):  # records that are not scored at all
        assert (dev[m] == c).all() and np.isneginf(res["x1"][m]).all() and np.isnan(res["x2"][m]).all(), where
        assert (mm[m] == 1).all() and (n[m] == 1).all(), where
    return ok


SETTINGS = {
    "defaults": dict(edge_threshold=0.97, ov_threshold=0.9),
    "merge_contigs_negative_thresholds": dict(edge_threshold=-1.0, ov_threshold=-1.0, merge_contigs=0.05),
    "merge_contigs_decides": dict(edge_threshold=0.9999, ov_threshold=-1.0, merge_contigs=0.02),
}


def _reference(oracle, n_quals, invalid, setting):
    key = (n_quals, invalid, setting)
    if key not in _cache:
        reads = _reads(n_quals, invalid)
        cand, skip = _candidates(reads.n_reads)
        st = hc.Settings(**SETTINGS[setting])
        ref = oracle.score_batch(reads, st, cand)
        for a in (cand, skip, ref):
            a.flags.writeable = False
        _cache[key] = (reads, cand, skip, st, ref)
    return _cache[key]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("invalid", ["qual", "base"])
@pytest.mark.parametrize("form", ["registers", "dma"])
@pytest.mark.parametrize("n_quals", [6, 35, 70])
def test_every_form_against_the_oracle(oracle, monkeypatch, n_quals, form, invalid, setting):
    reads, cand, skip, st, ref = _reference(oracle, n_quals, invalid, setting)
    if form == "dma":
        monkeypatch.setenv("HC_COOP_DMA_MIN", "1")
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        info = sc.kernel_info(cand.size)
        assert "score_kernel_coop<" + ("uint16_t" if n_quals > 60 else "uint8_t") in info, info
        if n_quals <= 60:  # (16-bit symbols have no LDS-DMA form)
            assert (", 0, true>" in info.split(" encoding=")[0]) == (form == "dma"), info
        res = sc.score_cands(_compact(sc, cand, skip))
        _, _, cls = sc.finalize(res, allow_errors=True)
    ok = _check(ref, res, cls, skip, f"{n_quals} quality values, {form}, invalid {invalid}, {setting}")
    seen = set(np.unique(ref["cls"][ok]).tolist())  # (the oracle's classes: what the settings are meant to exercise)
    if setting == "defaults":
        assert 0 in seen, seen
        rescanned = ~skip & np.isin(cand["read1"], [7, N_SINGLE + 9]) & (ref["status"] < 0) & (ref["status"] > -10)
        assert rescanned.sum() > 20, "the invalid symbols are meant to sit inside scored windows"
    elif setting == "merge_contigs_negative_thresholds":
        assert seen == {2}, seen  # every score passes a negative edge threshold
    else:
        assert 1 in seen, seen    # not an edge, not within merge_contigs: the negative overlap threshold admits it as a non-edge


@pytest.mark.parametrize("form", ["registers", "dma"])
@pytest.mark.parametrize("n_quals", [6, 35, 70])
def test_row_sink_launch(oracle, monkeypatch, n_quals, form):
    import torch

    reads, cand, skip, st, ref = _reference(oracle, n_quals, "qual", "defaults")
    if form == "dma":
        monkeypatch.setenv("HC_COOP_DMA_MIN", "1")
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        cd = _compact(sc, cand, skip)
        d_in = torch.from_numpy(cd.view(np.uint8).reshape(-1).copy()).cuda()
        d_out = torch.empty(cd.size * 24, dtype=torch.uint8, device="cuda")
        payload = torch.full((cd.size + 1, 4), -1, dtype=torch.int64, device="cuda")
        base = 1 << 33
        sc.score_pack_device(d_in.data_ptr(), cd.size, d_out.data_ptr(), cd.size, base, payload.data_ptr(), None, REC_COMPACT)
        sc.synchronize()
        res = d_out.cpu().numpy().view(hc.RESULT_DTYPE)
        _, _, cls = sc.finalize(res, allow_errors=True)
    _check(ref, res, cls, skip, f"row sink, {n_quals} quality values, {form}")
    p = payload.cpu().numpy()
    kept = np.nonzero(result_cls(res) != 0)[0]
    assert int(p[0, 0]) == kept.size
    rows = p[1:1 + kept.size]
    rows = rows[np.argsort(rows[:, 0])]
    assert np.array_equal(rows[:, 0], kept + base)
    assert np.array_equal(rows[:, 1], res["x1"][kept].view(np.int64)) and np.array_equal(rows[:, 2], res["x2"][kept].view(np.int64))
    assert np.array_equal(rows[:, 3], res["mm"][kept].astype(np.int64) | (res["n_cls"][kept].astype(np.int64) << 32))


def test_mixed_lengths_through_the_bucketed_launch(oracle, monkeypatch):
    monkeypatch.setenv("HC_BALANCE", "1")
    rng = np.random.default_rng(77)
    genome = ACGT[rng.integers(0, 4, 3000)]
    alphabet = (33 + np.arange(2, 8)).astype(np.uint8)
    lens = np.concatenate([[150, 1200], rng.integers(150, 1201, 38)])
    singles = []
    for ln in lens:
        s = int(rng.integers(0, 3000 - ln + 1))
        seq = bytearray(genome[s:s + ln].tobytes())
        singles.append((seq, alphabet[rng.integers(0, 6, ln)].tobytes()))
    singles[4][0][30] = ord("N")
    singles[6][0][60] = ord("X")
    reads = hc.ReadSet.from_lists([(bytes(a), b) for a, b in singles], [])
    cand, skip = _candidates(reads.n_reads, n=2000, max_pos=1200, seed=9)
    cand["ord"][cand["ord"] != ord("x")] = ord("-")
    st = hc.Settings(edge_threshold=0.97, ov_threshold=0.9)
    ref = oracle.score_batch(reads, st, cand)
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        assert "length-bucketed" in sc.kernel_info(cand.size), sc.kernel_info(cand.size)
        res = sc.score_cands(_compact(sc, cand, skip))
        _, _, cls = sc.finalize(res, allow_errors=True)
    _check(ref, res, cls, skip, "40 singles of 150..1 200 bp, bucketed")
