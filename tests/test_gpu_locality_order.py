"""The locality order (csrc/hc_locality.hip): launches of a regular store score the runs of equal smaller read id in the order of their
reads' minimisers, and the ticket form deals the items by XCD.  Only the order of processing changes: every record must come out
bit-identical to the plain launch (HC_LOCALITY=0) and to the oracle, whatever the order the batch arrives in."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import synth
from haploconduct_amd.records import REC_COMPACT, RESULT_DTYPE
from tests import _oracle

pytestmark = pytest.mark.gpu


def minimiser_order(reads, k=16):
    """numpy restatement of the device key: per read, the smallest (2-bit 16-mer * 0x9E3779B97F4A7C15 mod 2^64) >> 20 over its first
    sequence (A C G T = 0 1 2 3, anything else 0); reads sorted by it, ties in read order."""
    bases = np.asarray(reads.bases)
    off = np.asarray(reads.seq_off).astype(np.int64)
    first = np.asarray(reads.read_first_seq).astype(np.int64)
    lut = np.zeros(256, np.uint64)
    for ch, v in zip(b"ACGT", range(4)):
        lut[ch] = v
    keys = np.full(reads.n_reads, (1 << 44) - 1, np.uint64)
    for r in range(reads.n_reads):
        s = bases[off[first[r]]:off[first[r] + 1]]
        if s.size < k:
            continue
        code = lut[s]
        km = np.zeros(s.size - k + 1, np.uint64)
        for j in range(k):
            km = (km << np.uint64(2)) | code[j:s.size - k + 1 + j]
        with np.errstate(over="ignore"):
            keys[r] = ((km * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(20)).min()
    return np.argsort(keys, kind="stable").astype(np.uint32)


def test_the_order_is_the_minimiser_of_mate_1():
    reads, _ = synth.make_paired_dataset(3000, 6000, flip_frac=0.25, seed=21)
    with hc.EdgeScorer(hc.Settings(edge_threshold=0.97, min_overlap_len=150)) as sc:
        sc.set_reads(reads)
        got = sc.locality_order()
    assert np.array_equal(got, minimiser_order(reads))


def _device_scores(torch, sc, cd, locality, monkeypatch):
    if locality:
        monkeypatch.setenv("HC_LOCALITY", "1")
        monkeypatch.setenv("HC_LOCALITY_MIN", "1")  # the C2 sizes are below the default threshold
    else:
        monkeypatch.setenv("HC_LOCALITY", "0")
    d_in = torch.from_numpy(cd.view(np.uint8).reshape(-1)).cuda()
    d_out = torch.full((cd.size * 24,), 0xA5, dtype=torch.uint8, device="cuda")  # a pattern: a record not written shows
    torch.cuda.synchronize()  # the context's stream does not wait for torch's: the fill must have landed before the kernel writes
    sc.score_cands_device(d_in.data_ptr(), cd.size, d_out.data_ptr())
    sc.synchronize()
    return d_out.cpu().numpy().tobytes()


def _order(cand, order):
    if order == "grouped":
        return cand[np.argsort(cand["read1"], kind="stable")]
    if order == "shuffled":
        return cand[np.random.default_rng(5).permutation(cand.size)]
    return cand


@pytest.mark.parametrize("workload", ["c2", "c3-lite"])
@pytest.mark.parametrize("order", ["sfo", "grouped", "shuffled"])
def test_locality_launch_is_bit_identical(oracle, monkeypatch, workload, order):
    import torch

    import bench

    reads, cand, _, st = bench.build_workload(workload, 0)
    cand = _order(cand, order)
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        assert sc.locality_order().size == reads.n_reads
        cd = sc.pack_cands(cand)
        on = _device_scores(torch, sc, cd, True, monkeypatch)
        off = _device_scores(torch, sc, cd, False, monkeypatch)
        assert on == off, f"{workload} / {order}: the locality launch differs from the plain launch"
    # and against the oracle on a stretch of each end of the batch
    res = np.frombuffer(on, RESULT_DTYPE)
    for part in (slice(0, 20000), slice(cand.size - 20000, cand.size)):
        ref = _oracle.score_batch(reads, st, cand[part])
        got = res[part]
        assert np.array_equal(got["x1"].view(np.uint64), ref["x1"].view(np.uint64))
        assert np.array_equal(got["x2"].view(np.uint64), ref["x2"].view(np.uint64))
        assert np.array_equal(got["mm"], ref["mm"])


def test_time_kernel_and_repeat_launches_agree(monkeypatch):
    """Launch after launch on one context (the index scratch is reused, the flag re-zeroed): a grouped batch after a shuffled one and
    back."""
    import torch

    import bench

    reads, cand, _, st = bench.build_workload("c2", 0)
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        cd = sc.pack_cands(cand)
        cs = sc.pack_cands(_order(cand, "shuffled"))
        a = _device_scores(torch, sc, cd, True, monkeypatch)
        s1 = _device_scores(torch, sc, cs, True, monkeypatch)
        b = _device_scores(torch, sc, cd, True, monkeypatch)
        s0 = _device_scores(torch, sc, cs, False, monkeypatch)
        assert a == b and s1 == s0
        d_in = torch.from_numpy(cd.view(np.uint8).reshape(-1)).cuda()
        d_out = torch.empty(cd.size * 24, dtype=torch.uint8, device="cuda")
        assert sc.time_kernel(d_in.data_ptr(), cd.size, d_out.data_ptr(), 3, REC_COMPACT) > 0
        assert d_out.cpu().numpy().tobytes() == a


def test_read_set_with_singles_is_not_regular_and_stays_exact(oracle, monkeypatch):
    import torch

    reads, meta = synth.make_single_dataset(20000, 30000, len_lo=100, len_hi=250, n_strains=2, seed=9)
    cand = synth.single_candidates(meta, min_overlap=80, n_candidates=400000)
    st = hc.Settings(edge_threshold=0.97, min_overlap_len=80)
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        assert sc.locality_order().size == 0  # lengths differ: not a regular store, no order
        cd = sc.pack_cands(cand)
        on = _device_scores(torch, sc, cd, True, monkeypatch)
        off = _device_scores(torch, sc, cd, False, monkeypatch)
        assert on == off
    res = np.frombuffer(on, RESULT_DTYPE)[:20000]
    ref = _oracle.score_batch(reads, st, cand[:20000])
    assert np.array_equal(res["x1"].view(np.uint64), ref["x1"].view(np.uint64))
    assert np.array_equal(res["mm"], ref["mm"])
