#!/usr/bin/env python3
"""Times hc_set_reads_from_fastq_text (include/hcedge.h: the FASTQ files' text read on the device) against the route a caller has without
it: hc_host_fastq_load on 16 threads (HC_FASTQ_THREADS=16) followed by hc_set_reads, on the same files, and hc_ec_open with
hc_ec_fastq_on_device on and off.

Workloads (bases ACGT, qualities from 40 values, ids of seven digits), written to --dir once:
  singles  --reads single-end reads of 150 bases;
  pairs    --reads / 2 pairs of 2 x 150 (config 3's read set);
  long     --long reads of 10 000 bases.
The two routes alternate in one process, each on its own context; the first repetition of each checks the device's arrays against the
host reader's and is not timed.  Medians of --reps; the host route's min - max spread is reported with it, and the device route counts
as faster only where its median lies below the host route's by more than three times that spread.  One JSON line per workload and
measurement (the table of profiles/fastq_reader.md is those lines' figures).

    python tools/fastq_reader_bench.py [--reads 1000000] [--long 10000] [--reps 5] [--dir DIR] [--only K] [--no-stage]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HC_FASTQ_THREADS", "16")
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import _native as N  # noqa: E402
from haploconduct_amd import fastq_reader as FR  # noqa: E402
from haploconduct_amd import host  # noqa: E402


def fastq_bytes(n, length, first_id, seed):
    """n records of one length, ids first_id .. (seven digits), as one array of bytes"""
    rng = np.random.default_rng(seed)
    head = 1 + 7 + 1
    rec = head + length + 3 + length + 1
    a = np.empty((n, rec), np.uint8)
    a[:, 0] = ord("@")
    ids = np.arange(first_id, first_id + n, dtype=np.int64)
    for d in range(7):
        a[:, 7 - d] = 48 + (ids // 10 ** d) % 10
    a[:, 8] = 10
    a[:, head:head + length] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, length), dtype=np.uint8)]
    a[:, head + length:head + length + 3] = np.frombuffer(b"\n+\n", np.uint8)
    a[:, head + length + 3:rec - 1] = rng.integers(35, 75, (n, length), dtype=np.uint8)
    a[:, rec - 1] = 10
    return a.reshape(-1)


def host_route(ctx, paths):
    """hc_host_fastq_load + hc_set_reads + hc_host_fastq_free; -> (ms load, ms set_reads, view fields for the check)"""
    h, v = C.c_void_p(), host.hc_fastq_view()
    t0 = time.perf_counter()
    N.check(N.lib.hc_host_fastq_load(C.byref(h), C.byref(paths), C.byref(v)), "hc_host_fastq_load")
    t1 = time.perf_counter()
    N.check(N.lib.hc_set_reads(ctx, v.bases, v.quals, v.seq_off, v.read_first_seq, v.n_reads), "hc_set_reads")
    t2 = time.perf_counter()
    ids = np.ctypeslib.as_array(C.cast(v.read_ids, C.POINTER(C.c_uint64)), shape=(v.n_reads,)).copy()
    off = np.ctypeslib.as_array(C.cast(v.seq_off, C.POINTER(C.c_uint64)), shape=(v.n_seq + 1,)).copy()
    N.lib.hc_host_fastq_free(h)
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, ids, off


def summary(name, what, host_ms, dev_ms, extra=None):
    hm, dm = statistics.median(host_ms), statistics.median(dev_ms)
    spread = max(host_ms) - min(host_ms)
    out = {"workload": name, "measure": what, "host_ms_each": [round(x, 3) for x in host_ms], "device_ms_each": [round(x, 3) for x in dev_ms],
           "host_median_ms": round(hm, 3), "host_spread_ms": round(spread, 3), "device_median_ms": round(dm, 3),
           "device_faster_by_the_rule": bool(dm < hm - 3 * spread), "version": hc.version()}
    out.update(extra or {})
    return out


def run(name, files, reps, stage):
    s, p1, p2 = files
    paths = host.make_paths(s, p1, p2, None)
    host_ms, load_ms, set_ms, dev_ms, parts = [], [], [], [], []
    with hc.EdgeScorer() as dev, hc.EdgeScorer() as ref:
        for rep in range(reps + 1):
            lo, se, ids, off = host_route(ref._ctx, paths)
            t0 = time.perf_counter()
            cn = dev.set_reads_from_fastq(s, p1, p2)
            d = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                got = dev.fastq_fetch()
                assert np.array_equal(got[0], ids) and np.array_equal(got[1], off) and cn.n_host_ids == 0, name + ": the device's arrays differ"
                assert dev.info() == ref.info() and dev.kernel_info() == ref.kernel_info()
                continue
            host_ms.append(lo + se), load_ms.append(lo), set_ms.append(se), dev_ms.append(d)
            parts.append((cn.ms_copy, cn.ms_device, cn.ms_plan))
    extra = {"reads": int(cn.n_reads), "file_bytes": sum(os.path.getsize(f) for f in files if f), "reps": reps,
             "host_load_median_ms": round(statistics.median(load_ms), 3), "host_set_reads_median_ms": round(statistics.median(set_ms), 3),
             "device_ms[copy, device, plan]": [round(statistics.median(c), 3) for c in zip(*parts)]}
    print(json.dumps(summary(name, "hc_set_reads_from_fastq_text against hc_host_fastq_load (16 threads) + hc_set_reads", host_ms, dev_ms, extra)), flush=True)
    if not stage:
        return
    ov = os.path.join(os.path.dirname(s or p1), "empty_overlaps.txt")
    open(ov, "w").close()
    st = hc.Settings(n_threads=16)
    t = {False: [], True: []}
    host.keep_devices(True)
    try:
        for rep in range(reps + 1):
            for on in (False, True):
                host.fastq_on_device(on)
                t0 = time.perf_counter()
                ec = host.EdgeCalculatorStage(st, singles=s, paired1=p1, paired2=p2, overlaps=ov, output_dir=os.path.dirname(ov) + "/")
                d = (time.perf_counter() - t0) * 1e3
                assert ec.fastq_was_on_device() == on and ec.read_count() == cn.n_reads
                ec.close()
                if rep:
                    t[on].append(d)
    finally:
        host.fastq_on_device(False)
        host.keep_devices(False)
    print(json.dumps(summary(name, "hc_ec_open, hc_ec_fastq_on_device off against on (parked devices)", t[False], t[True])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--long", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir")
    ap.add_argument("--only", type=int, help="run workload K of the three alone")
    ap.add_argument("--no-stage", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        def write(name, *args):
            fastq_bytes(*args).tofile(os.path.join(d, name))
            return os.path.join(d, name)

        todo = [(f"{a.reads} single-end reads of 150", lambda: (write("s150.fastq", a.reads, 150, 1000000, 1), None, None)),
                (f"{a.reads // 2} pairs of 2 x 150", lambda: (None, write("p1.fastq", a.reads // 2, 150, 1000000, 2), write("p2.fastq", a.reads // 2, 150, 1000000, 3))),
                (f"{a.long} reads of 10000", lambda: (write("long.fastq", a.long, 10000, 1000000, 4), None, None))]
        for name, mk in todo if a.only is None else todo[a.only:a.only + 1]:
            run(name, mk(), a.reps, not a.no_stage)


if __name__ == "__main__":
    main()
