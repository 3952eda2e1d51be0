#!/usr/bin/env python3
"""Times hc_sr_originals_next and hc_sr_originals_write_text + fetch on one GPU against the route a caller had before them: the same
tables through the host mirror hc_host_sr_originals_next on one thread and on 16, followed by hc_host_sr_originals_text.

Workloads (tables written directly, as a merge call would return them: the call reads nothing else):
  cliques  --cliques super-reads of 3 to 40 vertices (tools/clique_next_bench.py's sizes and weights) over disjoint vertices, half the
           reads paired, a quarter of the paired cliques self-merged, a tenth more vertices as trivials; the dict with 1 entry per read
           and first_it (the first iteration) and with --dict entries per read, first_it off (a late iteration);
  pairs    --pairs two-vertex super-reads, dicts of 1, first_it.
Every repetition reloads the dict (hc_sr_originals_load, not timed).  The first repetition checks the device against the mirror
(offsets, entries, statuses, text) and is not timed.  Medians of --reps; one JSON line per workload (the table of
profiles/originals.md is those lines' figures).

    python tools/originals_bench.py [--cliques 20000] [--dict 50] [--pairs 1000000] [--reps 5] [--only K]
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
from haploconduct_amd import host  # noqa: E402
from haploconduct_amd import merge_next as MN  # noqa: E402
from haploconduct_amd import originals as OR  # noqa: E402
from haploconduct_amd.consensus import SR_LAYOUT_DTYPE  # noqa: E402
from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402


def workload(sizes, dict_size, first_it, trivial_share, seed=1):
    """-> (off, entries, originals.Tables): super-read i owns the vertices [start_i, start_i + sizes[i]), then the trivials' vertices"""
    rng = np.random.default_rng(seed)
    n = sizes.size
    n_sub = int(sizes.sum())
    nv = n_sub + int(trivial_share * n_sub)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    owner = np.repeat(np.arange(n), sizes)
    paired_clique = rng.random(n) < 0.5
    paired_read = np.concatenate([paired_clique[owner], rng.random(nv - n_sub) < 0.5])
    self_merged = paired_clique & (rng.random(n) < 0.25)
    kind = np.where(self_merged, MN.MN_SINGLE_SELF, np.where(paired_clique, MN.MN_PAIRED, MN.MN_SINGLE)).astype(np.uint32)
    overlap_pos = np.where(self_merged, rng.integers(1, 120, n), -1).astype(np.int32)
    n_lay = np.where(paired_clique, 2, 1)
    first_layout = np.concatenate([[0], np.cumsum(n_lay)]).astype(np.uint64)
    layouts = np.zeros(int(first_layout[-1]), SR_LAYOUT_DTYPE)
    layouts["total_len"] = 300
    single = kind != MN.MN_PAIRED
    new_id = np.zeros(n, np.int32)
    new_id[single] = np.arange(int(single.sum()))
    n_triv = nv - n_sub
    new_id[~single] = int(single.sum()) + n_triv + np.arange(int((~single).sum()))
    order = np.concatenate([np.flatnonzero(single), np.flatnonzero(~single)]).astype(np.uint32)
    sub = np.zeros(n_sub, FNO_SUBREAD_DTYPE)
    rows_of = np.concatenate([np.arange(int(start[i]), int(start[i + 1])) for i in order]) if n else np.zeros(0, np.int64)
    sub["node"] = rows_of
    sub["index1"] = rng.integers(0, 300, n_sub)
    sub["startpos1"] = rng.integers(0, 4, n_sub)
    pr = paired_read[rows_of]
    sub["index2"] = np.where(pr, rng.integers(0, 300, n_sub) + np.where(self_merged[owner[rows_of]], overlap_pos[owner[rows_of]], 0), -1)
    sub["startpos2"] = np.where(pr, rng.integers(0, 4, n_sub), -1)
    subread_off = np.concatenate([[0], np.cumsum(sizes[order])]).astype(np.uint64)
    state = np.concatenate([np.full(n_sub, MN.MN_V_MERGED), np.full(n_triv, MN.MN_V_TRIVIAL)]).astype(np.uint32)
    nodes = np.zeros(nv, FNO_READ_DTYPE)
    nodes["len1"], nodes["len2"], nodes["paired"] = 150, np.where(paired_read, 150, 0), paired_read
    nodes["id"][n_sub:] = int(single.sum()) + np.arange(n_triv)
    vertex_read = rng.permutation(nv).astype(np.uint32)
    vertex_fwd = (rng.random(nv) < 0.7).astype(np.uint8)
    nodes["orientation"] = vertex_fwd
    # the dict: read r owns the originals r * dict_size ..., as many as it has; a paired read's are paired (no :801 assert)
    read_paired = np.zeros(nv, bool)
    read_paired[vertex_read] = paired_read
    entries = np.zeros(nv * dict_size, OR.ORIGINAL_DTYPE)
    entries["id"] = np.arange(nv * dict_size)
    entries["paired"] = np.repeat(read_paired, dict_size)
    entries["forward"] = 1 if first_it else rng.random(entries.size) < 0.5
    entries["len1"] = 150
    entries["len2"] = np.where(entries["paired"], 150, 0)
    if not first_it:
        entries["index1"] = rng.integers(-20, 2000, entries.size)
        entries["index2"] = np.where(entries["paired"], rng.integers(-20, 2000, entries.size), 0)
    off = (np.arange(nv + 1) * dict_size).astype(np.uint64)
    t = OR.Tables(kind, new_id, overlap_pos, first_layout, layouts, order, subread_off, sub, state, nodes, vertex_read, vertex_fwd, n + n_triv, first_it)
    return off, entries, t


def run(name, off, entries, t, reps, host_reps):
    n_reads = off.size - 1
    # (the dict is loaded for the store's number of reads: a store of as many ten-base reads)
    b = np.tile(np.frombuffer(b"ACGTACGTAC", np.uint8), n_reads)
    q = np.full(b.size, ord("I"), np.uint8)
    store = ReadSet(b, q, (np.arange(n_reads + 1) * 10).astype(np.uint64), np.arange(n_reads + 1, dtype=np.uint32), np.arange(n_reads, dtype=np.uint64))
    dev_rows, host_rows = [], {1: [], 16: []}
    with hc.EdgeScorer() as sc:
        sc.set_reads(store)
        ref = None
        for rep in range(reps + 1):
            sc.sr_originals_load(off, entries)
            t0 = time.perf_counter()
            res = sc.sr_originals_next(t, None, None, None)
            t1 = time.perf_counter()
            text, ms_text_dev = OR.text(sc._ctx)
            t2 = time.perf_counter()
            if rep == 0:
                ref = host.sr_originals_next(off, entries, t)
                kept = sc.sr_originals_fetch()
                assert res.off.tolist() == ref.off.tolist() and res.status.tolist() == ref.status.tolist()
                assert kept[1].tobytes() == ref.entries.tobytes() and text == host.sr_originals_text(ref.off, ref.entries)
            else:
                whole = (t1 - t0) * 1e3
                dev_rows.append((whole, res.ms_device, res.ms_copy, whole - res.ms_device - res.ms_copy, (t2 - t1) * 1e3, ms_text_dev))
    for nt in (1, 16):
        for rep in range(host_reps):
            t0 = time.perf_counter()
            r = host.sr_originals_next(off, entries, t, n_threads=nt, cap=entries.size)  # (disjoint super-reads: no more entries than before)
            t1 = time.perf_counter()
            host.sr_originals_text(r.off, r.entries)
            t2 = time.perf_counter()
            host_rows[nt].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    med = statistics.median

    def cols(r):
        return [round(med(c), 3) for c in zip(*r)]

    return {"workload": name, "super_reads": int(t.sr_clique.size), "sources": int(t.subreads.size + t.vertex_read.size), "old_reads": int(n_reads),
            "old_entries": int(entries.size), "new_reads": int(t.new_read_count), "new_entries": int(ref.n_entries), "text_bytes": len(text), "reps": reps,
            "host_reps": host_reps, "device_ms[next whole, kernels+sort+scans (events), copies, other host, write_text+fetch whole, text kernels+scan (events)]":
            cols(dev_rows), "next_whole_ms_each": [round(r[0], 3) for r in dev_rows], "next_copies_ms_each": [round(r[2], 3) for r in dev_rows],
            "host_1_thread_ms[next, text]": cols(host_rows[1]), "host_16_threads_ms[next, text]": cols(host_rows[16]), "version": hc.version()}


CLIQUE_SIZES, CLIQUE_WEIGHTS = (3, 5, 8, 13, 16, 20, 30, 40), (.2, .2, .15, .15, .1, .1, .05, .05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cliques", type=int, default=20000)
    ap.add_argument("--dict", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--only", type=int, help="run workload 0, 1 or 2 alone (for a kernel trace of one of them)")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    sizes = rng.choice(CLIQUE_SIZES, a.cliques, p=CLIQUE_WEIGHTS)
    todo = [(f"{a.cliques} cliques, dicts of 1", (sizes, 1, True, 0.1)), (f"{a.cliques} cliques, dicts of {a.dict}", (sizes, a.dict, False, 0.1)),
            (f"{a.pairs} pairs, dicts of 1", (np.full(a.pairs, 2), 1, True, 0.1))]
    for name, args in todo if a.only is None else todo[a.only:a.only + 1]:
        print(json.dumps(run(name, *workload(*args), a.reps, a.host_reps)), flush=True)


if __name__ == "__main__":
    main()
