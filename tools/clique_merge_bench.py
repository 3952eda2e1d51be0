#!/usr/bin/env python3
"""Times the clique merge on the device graph (hc_sr_clique_merge) on one GPU, on a coverage-like input: --cliques cliques of 3 to 40
vertices (min_clique_size 4, so those above 12 go through filter_subreads), each a pile of 150-base reads (half of them 2 x 150 pairs) whose
starts fall within 100 bases of one another on one genome, with the base -> member records the layouts need.

  hc_sr_clique_merge   whole call by wall clock (one call, room given); of it the layout / filter / subread kernels, sorts and scans
                       (events), the host-decided filters, the consensus kernels (events) and the host-finished columns
  parent route         what a caller had before this call: hc_graph_fetch (80 bytes per record), the layouts and the filter on the host —
                       the mirror hc_host_sr_clique_merge_layouts on 16 threads, a block of cliques each, stands in for the caller's code —
                       and hc_sr_consensus with its upload of layouts and members

The first run warms the context and checks the routes against each other.  Medians of --reps runs; one JSON line (profiles/clique_merge.md holds its figures).

    python tools/clique_merge_bench.py [--cliques 20000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import consensus as SR  # noqa: E402
from haploconduct_amd import host  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402

M = 4
GAP = 120  # mate 2 starts this far behind mate 1


def workload(n_cliques, seed=1):
    """-> (reads, graph arrays, clique_off, clique_nodes, vertex_read, vertex_fwd): vertex v reads read v, all forward."""
    rng = np.random.default_rng(seed)
    sizes = rng.choice([3, 5, 8, 13, 16, 20, 30, 40], n_cliques, p=[.2, .2, .15, .15, .1, .1, .05, .05])
    off = np.zeros(n_cliques + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    V = int(off[-1])
    clique = np.repeat(np.arange(n_cliques), sizes)
    start = 600 * clique + rng.integers(0, 100, V)
    paired = rng.random(V) < 0.5
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 600 * n_cliques + 1000)]
    n_seq_of = 1 + paired.astype(np.int64)
    first = np.zeros(V + 1, np.int64)
    first[1:] = np.cumsum(n_seq_of)
    seq_start = np.repeat(start, n_seq_of)
    seq_start[first[:-1][paired] + 1] += GAP
    bases = genome[seq_start[:, None] + np.arange(150)[None, :]].ravel()
    flip = rng.random(bases.size) < 0.005  # read errors
    bases = np.where(flip, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, bases.size)], bases)
    quals = rng.integers(53, 74, bases.size).astype(np.uint8)
    reads = ReadSet(bases, quals, 150 * np.arange(seq_start.size + 1, dtype=np.uint64), first.astype(np.uint32), np.arange(V, dtype=np.uint64))
    # the base: the first single-end vertex of the clique, else its first vertex (src/SRBuilder.cpp:669-679)
    idx = np.arange(V)
    first_single = np.minimum.reduceat(np.where(paired, V, idx), off[:-1])
    base_of = np.where(first_single < off[1:], first_single, off[:-1])
    base = base_of[clique]
    node = idx[idx != base]
    b = base[node]
    e = np.zeros(node.size, host.EDGE_DTYPE)
    e["v1"], e["v2"], e["read1"], e["read2"] = b, node, b, node
    e["pos1"] = start[node] - start[b]
    e["pos2"] = np.where(paired[b] & paired[node], start[node] - start[b], np.where(paired[node], start[node] + GAP - start[b], 0))
    e["ori1"], e["ori2"], e["ord"], e["score"], e["perc"] = 1, 1, ord("1"), 1.0, 87
    out_off = np.zeros(V + 1, np.uint64)
    out_off[1:] = np.cumsum(np.bincount(b, minlength=V))
    in_off = np.zeros(V + 1, np.uint64)
    in_off[1:] = np.cumsum(np.bincount(node, minlength=V))
    in_nodes = b[np.argsort(node, kind="stable")].astype(np.uint32)
    nodes = np.concatenate([rng.permutation(np.arange(off[i], off[i + 1])) for i in range(n_cliques)]).astype(np.uint32)
    return reads, (e, out_off, in_nodes, in_off), off.astype(np.uint64), nodes, np.arange(V, dtype=np.uint32), np.ones(V, np.uint8)


def host_layouts(g, reads, off, nodes, vread, vfwd, threads=16):
    """The mirror on `threads` threads, a block of cliques each -> (layouts, members) of the USED members, and the filter classes."""
    n = off.size - 1
    cuts = np.linspace(0, n, threads + 1).astype(np.int64)
    st = SR.make_settings(min_clique_size=M)

    def block(k):
        a, b = cuts[k], cuts[k + 1]
        o = off[a:b + 1] - off[a]
        return SR.host_clique_merge_layouts(g["edges"], g["out_off"], reads, o, nodes[int(off[a]):int(off[b])], vread, vfwd, st)

    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(block, range(threads)))
    lay, mem, at = [], [], 0
    for p in parts:
        l, m = p.used_layouts()
        l["first_member"] += np.uint64(at)
        at += m.size
        lay.append(l)
        mem.append(m)
    return np.concatenate(lay), np.concatenate(mem), np.concatenate([p.layout_filter for p in parts])


def run(n_cliques, reps):
    reads, graph, off, nodes, vread, vfwd = workload(n_cliques)
    rows, parent = [], []
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        sc.graph_load(*graph)
        cap = None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            got = sc.sr_clique_merge(off, nodes, vread, vfwd, min_clique_size=M, cap=cap)
            t1 = time.perf_counter()
            g = sc.graph_fetch()
            p0 = time.perf_counter()
            layouts, members, classes = host_layouts(g, reads, off, nodes, vread, vfwd)
            p1 = time.perf_counter()
            cons = sc.sr_consensus(layouts, members, min_clique_size=M)
            p2 = time.perf_counter()
            if rep == 0:
                cap = int(got.result.out_off[-1])
                assert (got.clique_status == 0).all() and np.array_equal(got.layout_filter, classes)
                ul, um = got.used_layouts()
                assert np.array_equal(ul, layouts) and np.array_equal(um, members)
                assert np.array_equal(got.result.cons_seq, cons.cons_seq) and np.array_equal(got.result.cons_qual, cons.cons_qual)
                continue
            rows.append(((t1 - t0) * 1e3, got.ms_layout, got.ms_host_filter, got.result.ms_device, got.result.ms_host_finish))
            parent.append(((p0 - t1) * 1e3, (p1 - p0) * 1e3, (p2 - p1) * 1e3, (p2 - t1) * 1e3))
    med = statistics.median
    cols = lambda r: [round(med(c), 3) for c in zip(*r)]  # noqa: E731
    f = got.layout_filter
    return {"workload": "piles of 150-base reads, half of them pairs, min_clique_size 4", "cliques": n_cliques, "clique_entries": int(off[-1]),
            "records": int(graph[0].size), "layouts": int(got.layouts.size), "list_entries": int(got.members.size),
            "used_members": int(got.member_used.sum()), "positions": int(got.result.out_off[-1]), "filtered_layouts": got.n_filtered_layouts,
            "filter_classes[groups, stable, host]": [int((f == k).sum()) for k in (1, 2, 3)], "host_columns": got.result.n_host_columns, "reps": reps,
            "clique_merge_ms[whole, layout kernels, host filters, consensus kernels, host-finished columns]": cols(rows),
            "parent_route_ms[graph_fetch, mirror on 16 threads, hc_sr_consensus, whole]": cols(parent), "version": hc.version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cliques", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    r = run(a.cliques, a.reps)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
