#!/usr/bin/env python3
"""Times the edge merge on the device graph (hc_graph_merge_pairs, hc_sr_edge_merge) on one GPU: --pairs merges on a path-shaped graph
(vertex i -> i + 1, ids ascending along the path) over 150-base reads cut 20 bases apart from one genome, as single-end reads and as
2 x 150 paired reads.

  hc_graph_merge_pairs   whole call by wall clock; of it the target-column kernel (events), the copy and the host's walk
  hc_sr_edge_merge       whole call by wall clock (one call, room given); of it the kernels (events) and the host-finished columns
  parent route           single-end only: what a caller did before these calls — hc_graph_fetch (80 bytes per edge), the pairs picked and
                         their records gathered on the host (hc_host_graph_merge_pairs + numpy), hc_host_sr_edge_layouts, hc_sr_consensus.
                         The paired case had no route.

The first run warms the context and checks the routes against each other.  Medians of --reps runs; one JSON line per read type, and with
--markdown the table of profiles/edge_merge.md.

    python tools/edge_merge_bench.py [--pairs 1000000] [--reps 5] [--markdown profiles/edge_merge.md]
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
from haploconduct_amd.readstore import ReadSet  # noqa: E402


def workload(n_pairs, paired, seed=1):
    """-> (reads, graph arrays, vertex_read, vertex_fwd): 2 n_pairs vertices on a path over max(2000, n_pairs / 4) reads (a vertex reads
    read v mod n_reads; neighbours on the path are neighbours on the genome)."""
    rng = np.random.default_rng(seed)
    V = 2 * n_pairs
    n_reads = max(2000, n_pairs // 4)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20 * n_reads + 400)]
    n_seq = n_reads * (2 if paired else 1)
    start = 20 * np.arange(n_reads, dtype=np.int64)
    if paired:
        start = np.stack([start, start + 60], axis=1).ravel()
    bases = genome[start[:, None] + np.arange(150)[None, :]].ravel()
    flip = rng.random(bases.size) < 0.005  # read errors
    bases = np.where(flip, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, bases.size)], bases)
    quals = rng.integers(53, 74, bases.size).astype(np.uint8)
    seq_off = 150 * np.arange(n_seq + 1, dtype=np.uint64)
    first = np.arange(n_reads + 1, dtype=np.uint32) * (2 if paired else 1)
    reads = ReadSet(bases, quals, seq_off, first, np.arange(n_reads, dtype=np.uint64))
    vread = (np.arange(V) % n_reads).astype(np.uint32)
    e = np.zeros(V - 1, host.EDGE_DTYPE)
    e["v1"], e["v2"] = np.arange(V - 1), np.arange(1, V)
    e["read1"], e["read2"] = vread[:-1], vread[1:]
    # (the wrap from the last read to the first is no true overlap; its consensus is taken all the same)
    e["pos1"], e["pos2"], e["ori1"], e["ori2"], e["ord"], e["score"], e["perc"] = 20, 20, 1, 1, ord("1"), 1.0, 87
    out_off = np.minimum(np.arange(V + 1), V - 1).astype(np.uint64)
    in_off = np.maximum(np.arange(V + 1) - 1, 0).astype(np.uint64)
    in_nodes = np.arange(V - 1, dtype=np.uint32)
    return reads, (e, out_off, in_nodes, in_off), vread, np.ones(V, np.uint8)


def run(n_pairs, paired, reps):
    reads, graph, vread, vfwd = workload(n_pairs, paired)
    cap = n_pairs * (2 if paired else 1) * 340
    rows = {"merge_pairs": [], "edge_merge": [], "parent": []}
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        sc.graph_load(*graph)
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            pairs, st = sc.graph_merge_pairs(with_stats=True)
            t1 = time.perf_counter()
            got = sc.sr_edge_merge(pairs, vread, vfwd, cap=cap)
            t2 = time.perf_counter()
            parent = None
            if not paired:
                g = sc.graph_fetch()
                p0 = time.perf_counter()
                hp = host.graph_merge_pairs(g["edges"], g["out_off"])
                recs = g["edges"][g["out_off"][hp[:, 0]].astype(np.int64)]  # (a path: the pair's record is the source's only one)
                p1 = time.perf_counter()
                layouts, members = host.sr_edge_layouts(recs, reads)
                p2 = time.perf_counter()
                cons = sc.sr_consensus(layouts, members)
                p3 = time.perf_counter()
                parent = ((p0 - t2) * 1e3, (p1 - p0) * 1e3, (p2 - p1) * 1e3, (p3 - p2) * 1e3, (p3 - t2) * 1e3)
            if rep == 0:
                assert pairs.shape[0] == n_pairs and (got.pair_status == 0).all()
                if not paired:
                    assert np.array_equal(hp, pairs) and np.array_equal(got.layouts, layouts) and np.array_equal(got.members, members)
                    assert np.array_equal(got.result.cons_seq, cons.cons_seq) and np.array_equal(got.result.cons_qual, cons.cons_qual)
                continue
            rows["merge_pairs"].append(((t1 - t0) * 1e3, st["ms_kernel"], st["ms_copy"], st["ms_walk"]))
            rows["edge_merge"].append(((t2 - t1) * 1e3, got.result.ms_device, got.result.ms_host_finish))
            if parent:
                rows["parent"].append(parent)
    med = statistics.median

    def cols(r):
        return [round(med(c), 3) for c in zip(*r)] if r else None

    return {"workload": "path, " + ("2 x 150 paired" if paired else "150 single-end"), "pairs": n_pairs, "layouts": int(got.layouts.size),
            "positions": int(got.result.out_off[-1]), "host_columns": got.result.n_host_columns, "reps": reps,
            "merge_pairs_ms[whole, kernel, copy, walk]": cols(rows["merge_pairs"]),
            "edge_merge_ms[whole, kernels, host finish]": cols(rows["edge_merge"]),
            "parent_route_ms[graph_fetch, pick pairs, host layouts, hc_sr_consensus, whole]": cols(rows["parent"]), "version": hc.version()}


def markdown(results):
    s, p = results
    mp, em, pr = "merge_pairs_ms[whole, kernel, copy, walk]", "edge_merge_ms[whole, kernels, host finish]", \
        "parent_route_ms[graph_fetch, pick pairs, host layouts, hc_sr_consensus, whole]"
    lines = ["| part | single-end | 2 x 150 paired |", "|---|---|---|",
             f"| layouts / consensus positions | {s['layouts']} / {s['positions']} | {p['layouts']} / {p['positions']} |",
             f"| `hc_graph_merge_pairs`, whole call | {s[mp][0]} | {p[mp][0]} |",
             f"| — target-column kernel | {s[mp][1]} | {p[mp][1]} |", f"| — copy of targets and `out_off` | {s[mp][2]} | {p[mp][2]} |",
             f"| — host walk | {s[mp][3]} | {p[mp][3]} |", f"| `hc_sr_edge_merge`, whole call | {s[em][0]} | {p[em][0]} |",
             f"| — kernels and scans (events) | {s[em][1]} | {p[em][1]} |", f"| — host-finished columns | {s[em][2]} | {p[em][2]} |",
             f"| **resident route, both calls** | **{round(s[mp][0] + s[em][0], 3)}** | **{round(p[mp][0] + p[em][0], 3)}** |",
             f"| parent route: `hc_graph_fetch` | {s[pr][0]} | no route |", f"| — pairs picked, records gathered (host) | {s[pr][1]} | |",
             f"| — `hc_host_sr_edge_layouts` | {s[pr][2]} | |", f"| — `hc_sr_consensus` | {s[pr][3]} | |",
             f"| **parent route, whole** | **{s[pr][4]}** | |"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", help="write the figures' table to this file")
    a = ap.parse_args()
    results = []
    for paired in (False, True):
        results.append(run(a.pairs, paired, a.reps))
        print(json.dumps(results[-1]), flush=True)
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(markdown(results))


if __name__ == "__main__":
    main()
