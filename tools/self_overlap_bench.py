#!/usr/bin/env python3
"""Times the merge of self-overlapping paired super-reads (hc_sr_merge_self_overlaps, include/hcsr.h) on one GPU: 10^5 pairs of
2 x 150 bases of which none overlaps (every pair pays the whole scan), the same with half of them overlapping, and 10^4 pairs of
2 x 1,000.  Figures: the kernels (device events), the whole call from host arrays to host arrays, and the HOST MIRROR
(hc_host_sr_merge_self_overlaps: this project's restatement of SRBuilder::merge_self_overlap, not the reference's own loop) on 16
threads on the same box.  Every workload is compared with the mirror, scores as bit patterns, before it is timed.  Prints one JSON line
per workload.  (The reference's own function, one thread, on the first workload's kind of pairs:
tests/golden/make_golden_self_overlap.py --time, on the build machine only.)

    python tools/self_overlap_bench.py [--pairs 100000] [--long-pairs 10000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import host, synth  # noqa: E402


def best(f, reps):
    out, ts = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return out, min(ts)


def quality_alphabet():
    """The quality values of the SAVAGE example reads and their frequencies (a data file of the repository)."""
    with open(os.path.join(ROOT, "tests", "golden", "quality_histograms.json")) as f:
        h = json.load(f)["savage_singles"]["counts"]
    vals = np.array(sorted(int(k) for k in h), np.uint8)
    w = np.array([h[str(int(v))] for v in vals], np.float64)
    return vals, w / w.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--long-pairs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    qv, qw = quality_alphabet()
    work = [("2x150_none_overlapping", lambda: synth.make_mate_pairs(a.pairs, 150, 150, seed=1, qvals=qv, qweights=qw, overlap_frac=0.0)),
            ("2x150_half_overlapping", lambda: synth.make_mate_pairs(a.pairs, 150, 150, seed=2, qvals=qv, qweights=qw, overlap_frac=0.5, max_overlap=60)),
            ("2x1000_half_overlapping",
             lambda: synth.make_mate_pairs(a.long_pairs, 1000, 1000, seed=3, qvals=qv, qweights=qw, overlap_frac=0.5, max_overlap=60))]
    with hc.EdgeScorer() as sc:
        for name, make in work:
            seq, qual, pairs, _ = make()
            sc.sr_merge_self_overlaps(seq[:int(pairs[100]["off1"])], qual[:int(pairs[100]["off1"])], pairs[:100])  # tables, scratch
            dev, t_call = best(lambda: sc.sr_merge_self_overlaps(seq, qual, pairs), a.reps)
            ref, t16 = best(lambda: host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16), a.reps)
            same = all(np.array_equal(getattr(dev, k), getattr(ref, k)) for k in ("overlap_pos", "status", "out_off", "merged_seq", "merged_qual")) and \
                np.array_equal(dev.score.view(np.uint64), ref.score.view(np.uint64))
            print(json.dumps({"workload": name, "pairs": int(pairs.size), "merged": dev.n_merged, "offsets": dev.n_offsets, "host_pairs": dev.n_host_pairs,
                              "device_kernels_ms": round(dev.ms_device, 3), "device_host_share_ms": round(dev.ms_host, 3),
                              "device_call_with_copies_ms": round(t_call * 1e3, 3), "mirror_16_threads_ms": round(t16 * 1e3, 3),
                              "equal_to_mirror": bool(same)}), flush=True)
            assert same, name + ": the device result differs from the mirror"


if __name__ == "__main__":
    main()
