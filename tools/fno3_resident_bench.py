"""FNO=3 of a clique iteration, two routes on the dict that corresponds to tools/fno_bench.py's big_fno3 (2.5 * 10^5 super-reads, 10^6
originals, six per super-read), kept on the device over a store of reads with the same lengths:
  (a) what a caller had before hc_fno3_from_originals: hc_sr_originals_fetch, the per-read maps of an hc_fno3_input, hc_fno3_run;
  (b) hc_fno3_from_originals and the fetch of the whole text.
Medians of --reps runs and the spread (max - min) of each; a difference counts as a gain only if it exceeds three times the slower
route's spread (profiles/fastq_reader.md's rule).  Then a second input with one hub original shared by --hub reads (5 * 10^7
combinations at 10^4), route (b) only.  Prints one JSON line.
  python tools/fno3_resident_bench.py [--srs 250000] [--originals 1000000] [--hub 10000] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import fno as F  # noqa: E402
from haploconduct_amd import originals as OR  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402
from tools.fno_bench import big_fno3  # noqa: E402


def store_of(len1, len2, paired, seed=5):
    """random bases with these lengths, single-end reads first"""
    lens, first = [], np.zeros(len(len1) + 1, np.uint32)
    per = np.where(paired, 2, 1)
    first[1:] = np.cumsum(per)
    lens = np.zeros(int(first[-1]), np.int64)
    lens[first[:-1]] = len1
    lens[first[:-1][paired] + 1] = len2[paired]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    bases = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, total, dtype=np.uint8)]
    return ReadSet(bases, np.full(total, ord("I"), np.uint8), off, first, np.arange(len(len1), dtype=np.uint64))


def dict_of(inp):
    """big_fno3's maps as a dict over the reads in walk order (read r = srs[r]), entries ascending by id inside a read"""
    n = len(inp.srs)
    k = len(inp.originals) // n
    o = inp.originals.reshape(n, k)
    order = np.argsort(o["original_id"], axis=1, kind="stable")
    o = np.take_along_axis(o, order, axis=1)
    assert (np.diff(o["original_id"].astype(np.int64), axis=1) > 0).all()
    e = np.zeros(n * k, OR.ORIGINAL_DTYPE)
    flat = o.ravel()
    e["id"], e["index1"], e["index2"], e["len1"], e["len2"], e["paired"], e["forward"] = flat["original_id"], flat["index1"], flat["index2"], 100, 100, 1, 1
    return (np.arange(n + 1) * k).astype(np.uint64), e


def hub_dict(n, seed=7):
    """one original shared by all n reads, and one of its own each; the reads lie far apart, so few pairs write a line"""
    rng = np.random.default_rng(seed)
    e = np.zeros(2 * n, OR.ORIGINAL_DTYPE)
    e["id"][0::2], e["id"][1::2] = 0, 1 + np.arange(n)
    e["index1"] = rng.integers(0, 300000, 2 * n)
    e["len1"], e["forward"] = 100, 1
    return (2 * np.arange(n + 1)).astype(np.uint64), e


def med(xs):
    return round(statistics.median(xs), 3), round(max(xs) - min(xs), 3)


def route_a(sc, reads, counts3, n_originals):
    t0 = time.perf_counter()
    off, entries = sc.sr_originals_fetch()
    t1 = time.perf_counter()
    inp = F.Fno3Input.__new__(F.Fno3Input)
    o = np.zeros(len(entries), F.FNO_ORIGINAL_DTYPE)
    o["original_id"], o["index1"], o["index2"] = entries["id"], entries["index1"], entries["index2"]
    inp.srs, inp.counts = reads, (counts3[0], counts3[2], counts3[1])
    inp.orig_off, inp.originals = off, o
    inp.new_read_count, inp.original_readcount, inp.flags, inp.n_threads = len(reads), n_originals, 0, 0
    t2 = time.perf_counter()
    text, cnt = F.find_next_overlaps3(inp)
    t3 = time.perf_counter()
    return dict(fetch=(t1 - t0) * 1e3, maps=(t2 - t1) * 1e3, run=F.last_run_s * 1e3, total=(t3 - t0) * 1e3), text, cnt


def route_b(sc, counts3, n_originals):
    t0 = time.perf_counter()
    cn = OR.fno3_run(sc._ctx, counts3, n_originals)
    t1 = time.perf_counter()
    text = OR.fno3_text(sc._ctx, 0, cn["n_bytes"])
    t2 = time.perf_counter()
    return dict(call=(t1 - t0) * 1e3, ms_device=cn["ms_device"], fetch=(t2 - t1) * 1e3, total=(t2 - t0) * 1e3), text, cn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--srs", type=int, default=250_000)
    ap.add_argument("--originals", type=int, default=1_000_000)
    ap.add_argument("--hub", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    inp = big_fno3(a.srs, a.originals)
    n_single = inp.counts[0]
    counts3 = (n_single, 0, a.srs - n_single)
    reads = inp.srs.copy()
    reads["id"] = np.arange(a.srs)  # a read's id is its index in the store
    off, entries = dict_of(inp)
    res = {"super_reads": a.srs, "originals": a.originals, "reps": a.reps}
    with hc.EdgeScorer() as sc:
        sc.set_reads(store_of(reads["len1"], reads["len2"], reads["paired"] != 0))
        sc.sr_originals_load(off, entries)
        ta, tb = [], []
        route_a(sc, reads, counts3, a.originals), route_b(sc, counts3, a.originals)  # warm: allocations, the first launches
        for _ in range(a.reps):
            x, text_a, cnt_a = route_a(sc, reads, counts3, a.originals)
            y, text_b, cnt_b = route_b(sc, counts3, a.originals)
            ta.append(x), tb.append(y)
        assert cnt_a["candidates"] == cnt_b["candidates"], "the two routes list different pairs"
        cands = OR.fno3_candidates(sc._ctx, 0, cnt_b["candidates"])
        amb = int((cands["flags"] & OR.CAND_AMBIGUOUS != 0).sum())
        lines = lambda t: sorted(t.split(b"\n")[:-1])
        res["same_lines"] = bool(lines(text_a) == lines(text_b))  # (expected only where no pair is ambiguous)
        res["route_a_ms"] = {k: med([t[k] for t in ta]) for k in ta[0]}
        res["route_b_ms"] = {k: med([t[k] for t in tb]) for k in tb[0]}
        res["on_device_level_a"] = F.last_device_level
        res.update(candidates=cnt_b["candidates"], n_combos=cnt_b["n_combos"], combos_per_candidate=round(cnt_b["n_combos"] / max(1, cnt_b["candidates"]), 4),
                   n_ambiguous=amb, n_lines=cnt_b["n_lines"], n_bytes=cnt_b["n_bytes"])
        a_med, a_spread = res["route_a_ms"]["total"]
        b_med, b_spread = res["route_b_ms"]["total"]
        slower_spread = a_spread if a_med >= b_med else b_spread
        res["gain"] = bool(abs(a_med - b_med) > 3 * slower_spread)
        res["speedup_b_over_a"] = round(a_med / b_med, 2) if b_med else None
    if a.hub:
        n = a.hub
        off, entries = hub_dict(n)
        with hc.EdgeScorer() as sc:
            sc.set_reads(store_of(np.full(n, 300), np.zeros(n, np.int64), np.zeros(n, bool)))
            sc.sr_originals_load(off, entries)
            route_b(sc, (n, 0, 0), n + 1)
            th = [route_b(sc, (n, 0, 0), n + 1) for _ in range(max(3, a.reps // 2 + 1))]
            cn = th[-1][2]
            res["hub"] = {"reads": n, "n_combos": cn["n_combos"], "candidates": cn["candidates"], "n_lines": cn["n_lines"], "n_bytes": cn["n_bytes"],
                          "ms": {k: med([t[0][k] for t in th]) for k in th[0][0]}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
