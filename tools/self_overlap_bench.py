#!/usr/bin/env python3
"""Times the merge of self-overlapping paired super-reads (hc_sr_merge_self_overlaps, include/hcsr.h) on one GPU: 10^5 pairs of
2 x 150 bases of which none overlaps (every pair pays the whole scan), the same with half of them overlapping, and 10^4 pairs of
2 x 1,000.  Figures: the kernels (device events), the whole call from host arrays to host arrays, and the HOST MIRROR
(hc_host_sr_merge_self_overlaps: this project's restatement of SRBuilder::merge_self_overlap, not the reference's own loop) on 16
threads on the same box.  Every workload is compared with the mirror, scores as bit patterns, before it is timed.  Prints one JSON line
per workload.
The RESIDENT leg (hc_sr_merge_self_overlaps_kept) runs in the same run on the same batch: hc_sr_kept_load once, untimed, then the kept call
on the bytes it left on the device — its kernels, its host share and the whole call beside the host-input call's — and, as a chain, consensus
bytes -> self-merge -> next store by both routes: the host-input route pays the self-merge call from host arrays and hc_sr_set_next_reads
with the merged reads as extra bytes, the resident route the kept call and hc_sr_set_next_reads naming the merged reads among the kept
bytes.  (In both chains the consensus bytes are loaded once, untimed, in place of a consensus call; the host-input route's download of
them after that call is not counted either: it is charged less than it costs.)  (The reference's own function, one thread, on the first workload's kind of pairs:
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
from haploconduct_amd import next_reads as NR  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402


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
    tiny = ReadSet.from_lists(singles=[(b"ACGTACGTACGTACGTACGT", b"IIIIIIIIIIIIIIIIIIII")] * 4)  # a store for hc_sr_set_next_reads to replace
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        for name, make in work:
            seq, qual, pairs, _ = make()
            sc.sr_merge_self_overlaps(seq[:int(pairs[100]["off1"])], qual[:int(pairs[100]["off1"])], pairs[:100])  # tables, scratch
            dev, t_call = best(lambda: sc.sr_merge_self_overlaps(seq, qual, pairs), a.reps)
            ref, t16 = best(lambda: host.sr_merge_self_overlaps(seq, qual, pairs, n_threads=16), a.reps)
            same = all(np.array_equal(getattr(dev, k), getattr(ref, k)) for k in ("overlap_pos", "status", "out_off", "merged_seq", "merged_qual")) and \
                np.array_equal(dev.score.view(np.uint64), ref.score.view(np.uint64))
            # the resident leg: the same batch as kept bytes
            sc.sr_kept_load(seq, qual)
            sc.sr_merge_self_overlaps_kept(pairs[:100])  # scratch; what it appends is dropped by the next load
            ts, kept = [], None
            for _ in range(a.reps):
                sc.sr_kept_load(seq, qual)  # untimed
                t = time.perf_counter()
                kept = sc.sr_merge_self_overlaps_kept(pairs)
                ts.append(time.perf_counter() - t)
            t_kept = min(ts)
            rel = kept.relative()
            same_kept = all(np.array_equal(getattr(rel, k), getattr(ref, k)) for k in ("overlap_pos", "status", "out_off", "merged_seq", "merged_qual")) and \
                np.array_equal(rel.score.view(np.uint64), ref.score.view(np.uint64))
            # consensus bytes -> self-merge -> next store, by both routes
            merged = ref.status == 1
            keep_pairs = pairs[~merged]

            def entries(off, src):
                e = np.zeros(int(merged.sum()) + keep_pairs.size, NR.NEXT_ENTRY_DTYPE)
                m = np.flatnonzero(merged)
                e["off1"][:m.size], e["len1"][:m.size], e["kind"][:m.size], e["src1"][:m.size] = off[m], (off[m + 1] - off[m]), NR.NEXT_SINGLE, src
                for k in ("off1", "off2", "len1", "len2"):
                    e[k][m.size:] = keep_pairs[k]
                e["kind"][m.size:] = NR.NEXT_PAIRED
                return e

            def chain_host():
                r = sc.sr_merge_self_overlaps(seq, qual, pairs)
                return sc.sr_set_next_reads(entries(r.out_off, NR.SRC_BYTES), r.merged_seq, r.merged_qual)

            def chain_kept():
                r = sc.sr_merge_self_overlaps_kept(pairs)
                return sc.sr_set_next_reads(entries(r.out_off, NR.SRC_CONSENSUS))

            t_chain = {}
            for label, chain in (("host_input", chain_host), ("resident", chain_kept)):
                ts = []
                for _ in range(a.reps):
                    sc.set_reads(tiny)
                    sc.sr_kept_load(seq, qual)  # untimed: stands for the consensus call that left its bytes
                    t = time.perf_counter()
                    nxt = chain()
                    ts.append(time.perf_counter() - t)
                t_chain[label] = (min(ts), nxt.counts["n_kept"], nxt.counts["n_bytes"])
            same_chain = t_chain["host_input"][1:] == t_chain["resident"][1:]
            print(json.dumps({"workload": name, "pairs": int(pairs.size), "merged": dev.n_merged, "offsets": dev.n_offsets, "host_pairs": dev.n_host_pairs,
                              "device_kernels_ms": round(dev.ms_device, 3), "device_host_share_ms": round(dev.ms_host, 3),
                              "device_call_with_copies_ms": round(t_call * 1e3, 3), "mirror_16_threads_ms": round(t16 * 1e3, 3),
                              "equal_to_mirror": bool(same),
                              "kept_kernels_ms": round(kept.ms_device, 3), "kept_host_share_ms": round(kept.ms_host, 3), "kept_host_pairs": kept.n_host_pairs,
                              "kept_call_ms": round(t_kept * 1e3, 3), "kept_equal_to_mirror": bool(same_kept),
                              "chain_host_input_ms": round(t_chain["host_input"][0] * 1e3, 3), "chain_resident_ms": round(t_chain["resident"][0] * 1e3, 3),
                              "chain_next_reads": int(t_chain["resident"][1]), "chains_agree": bool(same_chain)}), flush=True)
            assert same, name + ": the device result differs from the mirror"
            assert same_kept, name + ": the kept call's result differs from the mirror"
            assert same_chain, name + ": the two routes keep different reads"


if __name__ == "__main__":
    main()
