#!/usr/bin/env python3
"""Times hc_sr_fastq_write_text / hc_sr_fastq_text_fetch (include/hcsr.h) against the route a caller had before them: hc_sr_next_reads_fetch
(the raw arrays through pageable memory) followed by the host mirrors hc_host_sr_fastq_text / hc_host_sr_fastq_tips_text on one thread.

Stores (bases ACGT, qualities from 40 values), each with no tips and with 10 % of its reads tips:
  singles  --reads single-end reads of 150 bases;
  pairs    the same bytes as --reads / 2 pairs of 2 x 150;
  long     --long reads of 10 000 bases.
Every repetition loads the store (hc_set_reads, not timed), then runs hc_sr_set_next_reads with one forward trivial entry per read that is
no tip — the next store's gather moves the same bytes with the same wave_copy as the write kernel, on the same store in the same run —,
then hc_sr_fastq_write_text with the tips (reads of the store that call read), the fetch of the four files, and the old route.  The first
repetition checks the device's four files against the mirrors and is not timed.  Medians of --reps; one JSON line per workload (the
table of profiles/fastq_text.md is those lines' figures).

The per-kernel times of profiles/fastq_text.md come from a kernel trace of this tool's run:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/fastq_text_bench.py
    python tools/fastq_text_bench.py --trace-csv DIR/.../*_kernel_trace.csv
prints, per kernel of interest, its dispatches' durations in dispatch order (workload after workload, --reps + 1 each).

    python tools/fastq_text_bench.py [--reads 1000000] [--long 10000] [--reps 5] [--only K]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import fastq_text as FQ  # noqa: E402
from haploconduct_amd import host  # noqa: E402
from haploconduct_amd import next_reads as NR  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402

KERNELS = ("sr_next_gather_kernel", "fq_sizes_kernel", "fq_write_kernel")


def make_store(n_reads, length, paired, seed=1):
    rng = np.random.default_rng(seed)
    n_seq = n_reads * (2 if paired else 1)
    total = n_seq * length
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total, dtype=np.uint8)]
    quals = rng.integers(35, 75, total, dtype=np.uint8)
    off = (np.arange(n_seq + 1, dtype=np.uint64) * np.uint64(length))
    first = (np.arange(n_reads + 1, dtype=np.uint32) * np.uint32(2 if paired else 1))
    return ReadSet(bases, quals, off, first, np.arange(n_reads, dtype=np.uint64))


def subset_bytes(store, reads):
    """bases and qualities of the named reads, in that order, forward: what the trivial entries leave (every read has as many bytes)"""
    return store.bases.reshape(store.n_reads, -1)[reads].reshape(-1), store.quals.reshape(store.n_reads, -1)[reads].reshape(-1)


def run(name, store, tip_share, reps):
    rng = np.random.default_rng(2)
    n = store.n_reads
    is_tip = rng.random(n) < tip_share
    tips = np.flatnonzero(is_tip).astype(np.uint32)  # vertex v is read v
    vertex_read = np.arange(n, dtype=np.uint32)
    kept = np.flatnonzero(~is_tip)
    entries = np.zeros(kept.size, NR.NEXT_ENTRY_DTYPE)
    entries["read"] = kept
    entries["kind"] = NR.NEXT_TRIVIAL_PAIRED if store.is_paired(0) else NR.NEXT_TRIVIAL
    rows, text_bytes, gather_bytes = [], 0, 0
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        for rep in range(reps + 1):
            sc.set_reads(store)
            res = sc.sr_set_next_reads(entries)
            assert not res.empty and res.counts["n_kept"] == kept.size
            gather_bytes = 2 * int(res.counts["n_bytes"])
            t0 = time.perf_counter()
            cn = FQ.write_text(sc._ctx, tips, vertex_read)
            t1 = time.perf_counter()
            files = [FQ.fetch(sc._ctx, f, 0, cn.n_bytes[f]) for f in range(4)]
            t2 = time.perf_counter()
            new = sc.sr_next_reads_fetch()
            t3 = time.perf_counter()
            mirror = [host.sr_fastq_text(new, f) for f in range(3)] + [host.sr_fastq_tips_text(store, tips)]
            t4 = time.perf_counter()
            if rep == 0:
                assert files == mirror, name + ": the device's files differ from the mirrors'"
                want = subset_bytes(store, kept)
                assert np.array_equal(new.bases, want[0]) and np.array_equal(new.quals, want[1])
                continue
            text_bytes = sum(len(f) for f in files)
            rows.append((cn.ms_device, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, res.counts["ms_device"]))
    cols = [round(statistics.median(c), 3) for c in zip(*rows)]
    return {"workload": name, "reads": n, "tips": int(tips.size), "text_bytes": text_bytes, "gather_bytes": gather_bytes, "reps": reps,
            "ms[write_text events, write_text whole, fetch of the four files, hc_sr_next_reads_fetch, mirrors on one thread, hc_sr_set_next_reads events]": cols,
            "write_text_events_ms_each": [round(r[0], 3) for r in rows], "fetch_ms_each": [round(r[2], 3) for r in rows],
            "old_route_ms_each": [round(r[3] + r[4], 3) for r in rows], "version": hc.version()}


def summarise_trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for k in KERNELS:
        ms = [round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, 4) for r in rows if k in r["Kernel_Name"]]
        print(json.dumps({"kernel": k, "dispatches": len(ms), "ms_each": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--long", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, help="run workload K of the six alone")
    ap.add_argument("--trace-csv", help="summarise a rocprofv3 kernel trace of a run of this tool instead of running")
    a = ap.parse_args()
    if a.trace_csv:
        return summarise_trace(a.trace_csv)
    stores = [(f"{a.reads} single-end reads of 150", lambda: make_store(a.reads, 150, False)),
              (f"{a.reads // 2} pairs of 2 x 150", lambda: make_store(a.reads // 2, 150, True)),
              (f"{a.long} reads of 10000", lambda: make_store(a.long, 10000, False))]
    todo = [(name + (", 10 % tips" if share else ", no tips"), mk, share) for name, mk in stores for share in (0.0, 0.1)]
    for name, mk, share in todo if a.only is None else todo[a.only:a.only + 1]:
        print(json.dumps(run(name, mk(), share, a.reps)), flush=True)


if __name__ == "__main__":
    main()
