"""How the ticket form's waves get their items and the locality order's index passes (hc_kernels.hip: score_kernel_coop, WQ;
hc_locality.hip: launch_locality_index) at the sizes where they can go wrong: a wave whose only item is partial, waves that take three
and more items with a partial last one, runs without records, a run longer than several items, ids out of range, batches that are not
grouped, scratch left behind by a larger launch, and a read set of more tiles of runs than a fill workgroup has lanes.  Only the order
of processing may change: every case compares the whole result buffer, pre-filled with a pattern, byte for byte with the plain launch
(HC_LOCALITY=0), and the first and the last 20 000 records with the oracle."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import synth
from haploconduct_amd.records import RESULT_DTYPE, result_cls
from tests import _oracle

pytestmark = pytest.mark.gpu

N_MANY = 800017  # 256 workgroups x 16 waves: 12 501 items, three and more per wave, the last one of 17 records
_cache = {}


def _dataset():
    if not _cache:
        reads, meta = synth.make_paired_dataset(9000, 3000, flip_frac=0.25, seed=31)
        cand = synth.paired_candidates(meta)  # sfo2overlaps order: grouped by the smaller read id
        assert cand.size >= N_MANY
        cand.flags.writeable = False
        _cache["d"] = (reads, cand, hc.Settings(edge_threshold=0.97, min_overlap_len=150))
    return _cache["d"]


def _hot(cand):
    return np.minimum(cand["read1"], cand["read2"]).astype(np.int64)


def _launch(torch, sc, cd, locality, monkeypatch):
    monkeypatch.setenv("HC_COOP_DMA_MIN", "1")  # the LDS-DMA ticket form at these sizes
    monkeypatch.setenv("HC_LOCALITY_MIN", "1")
    monkeypatch.setenv("HC_LOCALITY", "1" if locality else "0")
    info = sc.kernel_info(cd.size)
    assert ", 0, true>" in info.split(" encoding=")[0], info
    d_in = torch.from_numpy(cd.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((cd.size * 24,), 0xA5, dtype=torch.uint8, device="cuda")  # a pattern: a record not written shows
    torch.cuda.synchronize()  # the context's stream does not wait for torch's: the fill must have landed before the kernel writes
    sc.score_cands_device(d_in.data_ptr(), cd.size, d_out.data_ptr())
    sc.synchronize()
    return d_out.cpu().numpy().tobytes()


def _against_oracle(reads, st, cand, got_bytes, where):
    res = np.frombuffer(got_bytes, RESULT_DTYPE)
    parts = [slice(0, cand.size)] if cand.size <= 40000 else [slice(0, 20000), slice(cand.size - 20000, cand.size)]
    for part in parts:
        ref = _oracle.score_batch(reads, st, cand[part])
        got = res[part]
        ok = ref["status"] == 0
        assert np.array_equal(got["x1"].view(np.uint64)[ok], ref["x1"].view(np.uint64)[ok]), where + ": x1"
        assert np.array_equal(got["x2"].view(np.uint64)[ok], ref["x2"].view(np.uint64)[ok]), where + ": x2"
        assert np.array_equal(got["mm"][ok], ref["mm"][ok]), where + ": mm"
        assert (result_cls(got)[~ok] == 7).all(), where + ": a malformed record is an error"


def _both_ways(cand, monkeypatch, where, oracle_too=True, reads=None):
    import torch

    st = _dataset()[2]
    reads = _dataset()[0] if reads is None else reads
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        cd = sc.pack_cands(cand)
        on = _launch(torch, sc, cd, True, monkeypatch)
        off = _launch(torch, sc, cd, False, monkeypatch)
    assert len(on) == cand.size * 24
    assert on == off, where + ": the locality launch differs from the plain launch"
    if oracle_too:
        _against_oracle(reads, st, cand, on, where)
    return on


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025])
def test_a_waves_only_item_is_partial(oracle, monkeypatch, n):
    _, cand, _ = _dataset()
    _both_ways(cand[:n], monkeypatch, f"n = {n}")


def test_three_and_more_items_per_wave_and_a_partial_last_one(oracle, monkeypatch):
    _, cand, _ = _dataset()
    _both_ways(cand[:N_MANY], monkeypatch, f"n = {N_MANY}")


def test_ids_out_of_range_form_the_last_run(oracle, monkeypatch):
    reads, cand, _ = _dataset()
    c = cand[:70001].copy()
    c["read1"][-300:] = reads.n_reads + 3 + np.arange(300) % 5
    c["read2"][-300:] = reads.n_reads + 9
    c["read2"][-40:] = 0xFFFFFFF0
    assert (np.diff(np.minimum(_hot(c), reads.n_reads)) >= 0).all()
    _both_ways(c, monkeypatch, "ids out of range")


def test_reads_without_records_several_in_a_row(oracle, monkeypatch):
    reads, cand, _ = _dataset()
    c = cand[:150001]
    h = _hot(c)
    top = int(h.max())
    gone = (h < 7) | ((h >= 100) & (h < 140)) | (h == 141) | ((h >= top - 60) & (h < top)) | ((h % 64 == 5) & (h > 1000))
    c = c[~gone]
    assert c.size > 100000 and c.size % 64 != 0
    _both_ways(c, monkeypatch, "runs without records")


def test_one_read_owns_more_records_than_several_items(oracle, monkeypatch):
    _, cand, _ = _dataset()
    c = cand[:90001].copy()
    k0, k1 = 30011, 31111  # 1 100 records, 17 items and more, starting inside a 64-record block
    h = int(_hot(c)[k0])
    first_is_hot = c["read1"][k0:k1] <= c["read2"][k0:k1]
    c["read1"][k0:k1] = np.where(first_is_hot, h, c["read1"][k0:k1])
    c["read2"][k0:k1] = np.where(first_is_hot, c["read2"][k0:k1], h)
    hot = _hot(c)
    assert (np.diff(hot) >= 0).all() and (hot == h).sum() >= k1 - k0
    _both_ways(c, monkeypatch, "one long run")


def _ungrouped(cand, how):
    if how == "shuffled":
        return cand[np.random.default_rng(5).permutation(cand.size)]
    if how == "descending":
        return cand[::-1].copy()
    c = cand.copy()  # sorted but for one swapped pair of neighbours inside a 64-record block
    h = _hot(c)
    k = np.nonzero((h[:-1] != h[1:]) & (np.arange(h.size - 1) % 64 < 63) & (np.arange(h.size - 1) > 5000))[0][0]
    c[[k, k + 1]] = c[[k + 1, k]]
    assert _hot(c)[k] > _hot(c)[k + 1] and k // 64 == (k + 1) // 64
    return c


@pytest.mark.parametrize("how", ["shuffled", "descending", "one_swapped_pair"])
def test_a_batch_that_is_not_grouped(oracle, monkeypatch, how):
    _, cand, _ = _dataset()
    _both_ways(_ungrouped(cand[:100003], how), monkeypatch, how)


def test_a_grouped_batch_after_a_larger_ungrouped_one(oracle, monkeypatch):
    """One context: the smaller launch finds the larger one's boundaries, sums and permutation in the scratch."""
    import torch

    reads, cand, st = _dataset()
    big, small = _ungrouped(cand[:N_MANY], "shuffled"), cand[200000:200000 + 300001]
    with hc.EdgeScorer(st) as sc:
        sc.set_reads(reads)
        cb, cs = sc.pack_cands(big), sc.pack_cands(small)
        b_on = _launch(torch, sc, cb, True, monkeypatch)
        s_on = _launch(torch, sc, cs, True, monkeypatch)
        b_again = _launch(torch, sc, cb, True, monkeypatch)
        s_off = _launch(torch, sc, cs, False, monkeypatch)
        b_off = _launch(torch, sc, cb, False, monkeypatch)
    assert s_on == s_off, "the grouped batch after the larger ungrouped one differs from the plain launch"
    assert b_on == b_off and b_again == b_off
    _against_oracle(reads, st, small, s_on, "grouped after ungrouped")


def test_more_tiles_of_runs_than_a_workgroup_has_lanes(oracle, monkeypatch):
    """140 000 reads are 274 tiles of 512 runs: a fill workgroup adds up the sums in front of it in more than one turn of its 256 lanes."""
    reads, meta = synth.make_paired_dataset(140000, 500000, flip_frac=0.25, seed=33)
    cand = synth.paired_candidates(meta)
    assert reads.n_reads > 256 * 512 and cand.size > 10 ** 6
    _both_ways(cand, monkeypatch, "274 tiles", reads=reads)
