#!/usr/bin/env python3
"""Times consensus -> the next iteration's read store on one GPU, two ways, on edge merges of 150-base single-end reads.

  host route      what a caller did before hc_sr_set_next_reads: hc_sr_consensus with its copies to the host, the filters of process_cliques
                  and Read::test_N_rate on the host (numpy: an N count per super-read by a segmented sum, then one boolean gather — or no
                  copy at all when every super-read survives; this part is the caller's own code, so it is reported apart), the trivial super-reads appended, hc_set_reads from the host arrays
  resident route  hc_sr_keep_device on: hc_sr_consensus (its copies to the host stay: the call's contract), then hc_sr_set_next_reads on
                  the bytes it left on the device

Both routes end with the same store (checked before timing: the fetched raw arrays and hc_get_info).  Medians of --reps runs, one JSON line.

    python tools/next_reads_bench.py [--edges 1000000] [--reps 5] [--trivials 0.1]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import next_reads as NR  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402
from tools.consensus_bench import edge_merge_workload  # noqa: E402


def host_filter(reads, cons, trivial_reads):
    """The caller's work between hc_sr_consensus and hc_set_reads on the host route: (bases, quals, seq_off, read_first_seq)."""
    off = cons.out_off.astype(np.int64)
    lens = off[1:] - off[:-1]
    is_n = cons.cons_seq == ord("N")
    n_count = np.add.reduceat(is_n, np.minimum(off[:-1], max(is_n.size - 1, 0)), dtype=np.int64) if is_n.size else np.zeros(lens.size, np.int64)
    n_count[lens == 0] = 0  # (reduceat gives an empty segment the element it starts at)
    keep = (lens > 0) & (n_count.astype(np.float64) < 0.05 * lens.astype(np.float64))
    if keep.all():
        b, q = cons.cons_seq, cons.cons_qual
    else:
        m = np.repeat(keep, lens)
        b, q = cons.cons_seq[m], cons.cons_qual[m]
    klen = lens[keep]
    t_off = reads.seq_off.astype(np.int64)
    t_len = (t_off[1:] - t_off[:-1])[trivial_reads]
    if trivial_reads.size:  # (single-end reads of one length, forward)
        idx = (t_off[trivial_reads][:, None] + np.arange(int(t_len[0]))[None, :]).ravel()
        b, q = np.concatenate([b, reads.bases[idx]]), np.concatenate([q, reads.quals[idx]])
    seq_off = np.zeros(klen.size + t_len.size + 1, np.uint64)
    seq_off[1:] = np.cumsum(np.concatenate([klen, t_len]))
    first = np.arange(seq_off.size, dtype=np.uint32)
    return ReadSet(b, q, seq_off, first, np.arange(first.size - 1, dtype=np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trivials", type=float, default=0.1, help="share of the reads added as trivial super-reads")
    a = ap.parse_args()
    reads, layouts, members = edge_merge_workload(a.edges)
    trivial_reads = np.arange(0, reads.n_reads, max(1, int(round(1 / a.trivials))), dtype=np.int64) if a.trivials > 0 else np.zeros(0, np.int64)
    kw = dict(error_correction=False)
    t_host, t_res, parts_host, parts_res = [], [], [], []
    with hc.EdgeScorer() as sh, hc.EdgeScorer() as sr:
        sr.sr_keep_device(True)

        def entries_of(cons):
            off = cons.out_off.astype(np.int64)
            e = np.zeros(layouts.size + trivial_reads.size, NR.NEXT_ENTRY_DTYPE)
            e["off1"][:layouts.size], e["len1"][:layouts.size] = off[:-1], off[1:] - off[:-1]
            e["kind"][layouts.size:], e["read"][layouts.size:] = NR.NEXT_TRIVIAL, trivial_reads
            return e

        for rep in range(a.reps + 1):  # the first run warms both contexts and checks the two routes against each other
            sh.set_reads(reads)
            sr.set_reads(reads)
            t0 = time.perf_counter()
            cons = sh.sr_consensus(layouts, members, **kw)
            t1 = time.perf_counter()
            nxt = host_filter(reads, cons, trivial_reads)
            t2 = time.perf_counter()
            sh.set_reads(nxt)
            t3 = time.perf_counter()
            r0 = time.perf_counter()
            cons_r = sr.sr_consensus(layouts, members, **kw)
            r1 = time.perf_counter()
            e = entries_of(cons_r)
            r2 = time.perf_counter()
            res = sr.sr_set_next_reads(e)
            r3 = time.perf_counter()
            if rep == 0:
                got = sr.sr_next_reads_fetch()
                assert np.array_equal(got.bases, nxt.bases) and np.array_equal(got.quals, nxt.quals) and np.array_equal(got.seq_off, nxt.seq_off)
                assert sh.info() == sr.info() and res.counts["n_kept"] == nxt.n_reads
                continue
            t_host.append((t3 - t0) * 1e3)
            t_res.append((r3 - r0) * 1e3)
            parts_host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            parts_res.append(((r1 - r0) * 1e3, (r2 - r1) * 1e3, (r3 - r2) * 1e3, res.counts["ms_device"], res.counts["ms_plan"]))
    med = statistics.median

    def cols(rows):
        return [round(med(c), 3) for c in zip(*rows)]

    print(json.dumps({"workload": "edge_merge", "layouts": int(layouts.size), "positions": int(cons.out_off[-1]), "trivials": int(trivial_reads.size),
                      "next_reads": int(nxt.n_reads), "next_bytes": int(nxt.bases.size), "reps": a.reps,
                      "host_route_ms": round(med(t_host), 3), "host_route_parts_ms[consensus, host filter, set_reads]": cols(parts_host),
                      "resident_route_ms": round(med(t_res), 3),
                      "resident_route_parts_ms[consensus, entries, set_next_reads, of it kernels, of it planning]": cols(parts_res),
                      "version": hc.version()}))


if __name__ == "__main__":
    main()
