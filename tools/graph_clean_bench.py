#!/usr/bin/env python3
"""Times the four graph-cleaning calls on the device graph (hc_graph_remove_inclusions, hc_graph_remove_transitive,
hc_graph_remove_tips, hc_graph_remove_branches) and the fetch of branching_edges on an interval graph: reads tiled along
a genome, `--degree` out-edges per read, a tenth of the dead-end edges tips.  Every figure is the median of `--reps` runs,
each on a freshly loaded graph (the load is not timed), after one untimed warm-up run; the calls are synchronous, so wall
time around a call is the time of its kernels, its host steps and its counter read-backs together.

--mirror also times the host mirror (HostGraph, single-threaded: it restates the reference's loops) on the same graph,
once.  Prints one JSON line.

    python tools/graph_clean_bench.py --vertices 1000000 --degree 20 --mirror
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd.host import EDGE_DTYPE, READ_GEOM_DTYPE, HostGraph  # noqa: E402


def interval_graph(V, degree, seed):
    """Read i -> reads i + 1 .. i + degree (nine in ten of them), inserted in a random order; single-end reads of 250 bases."""
    rng = np.random.default_rng(seed)
    v1, v2 = [], []
    for d in range(1, degree + 1):
        a = np.arange(V - d, dtype=np.int64)
        ok = rng.random(V - d) < 0.9
        v1.append(a[ok])
        v2.append(a[ok] + d)
    v1, v2 = np.concatenate(v1), np.concatenate(v2)
    p = rng.permutation(v1.size)
    v1, v2 = v1[p], v2[p]
    n = v1.size
    e = np.zeros(n, EDGE_DTYPE)
    e["v1"], e["v2"], e["read1"], e["read2"] = v1, v2, v1, v2
    e["score"], e["perc"], e["ori1"], e["ori2"], e["ord"] = 1.0, 100, 1, 1, ord("-")
    kind = rng.random(n)
    ext = np.where(kind < 0.025, 0, np.where(kind < 0.1, rng.integers(1, 150, n), rng.integers(150, 240, n))).astype(np.int32)
    e["len1"] = e["len0"] = 250 - ext
    e["pos1"], e["pos4"] = ext, np.arange(n)
    order = np.argsort(v1, kind="stable")
    out_off = np.concatenate([[0], np.cumsum(np.bincount(v1, minlength=V))]).astype(np.uint64)
    in_order = np.argsort(v2, kind="stable")
    in_off = np.concatenate([[0], np.cumsum(np.bincount(v2, minlength=V))]).astype(np.uint64)
    incl = (rng.random(V) < 0.01).astype(np.uint8)
    geom = np.zeros(V, READ_GEOM_DTYPE)
    geom["len1"] = 250
    return e[order], out_off, v1[in_order].astype(np.uint32), in_off, incl, geom


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-tip-len", type=int, default=150)
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    edges, out_off, in_nodes, in_off, incl, geom = interval_graph(a.vertices, a.degree, a.seed)
    steps = ("remove_inclusions", "remove_transitive", "remove_tips", "remove_branches", "fetch_branching_edges")
    times = {k: [] for k in steps}
    counts = {}
    with hc.EdgeScorer(hc.Settings()) as sc:
        for rep in range(a.reps + 1):  # the first run warms up (allocations, code objects)
            sc.graph_load(edges, out_off, in_nodes, in_off, incl)
            t = {}
            t["remove_inclusions"], counts["inclusions"] = timed(sc.graph_remove_inclusions)
            t["remove_transitive"], counts["transitive"] = timed(lambda: sc.graph_remove_transitive(1, False))
            t["remove_tips"], counts["tips"] = timed(lambda: sc.graph_remove_tips(a.max_tip_len, geom))
            t["remove_branches"], counts["branches"] = timed(sc.graph_remove_branches)
            t["fetch_branching_edges"], be = timed(sc.graph_branching_edges)
            if rep:
                for k in steps:
                    times[k].append(t[k])
        n_branching = int(be.size)
    res = dict(vertices=a.vertices, edges=int(edges.size), reps=a.reps, n_branching_edges=n_branching, counts=counts,
               device_ms={k: round(1e3 * statistics.median(v), 3) for k, v in times.items()},
               device_ms_min_max={k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in times.items()})
    if a.mirror:
        g = HostGraph(a.vertices, hc.Settings())
        assert g.adopt(edges, out_off, in_nodes, in_off, incl) == 0
        m = {}
        m["remove_inclusions"], _ = timed(g.remove_inclusions)
        m["remove_transitive"], _ = timed(lambda: g.remove_transitive_edges(1, False))
        m["remove_tips"], mt = timed(lambda: g.remove_tips(a.max_tip_len, geom))
        m["remove_branches"], mb = timed(g.remove_branches)
        assert mt == counts["tips"] and {k: v for k, v in mb.items() if k != "cc_rounds"} == {k: v for k, v in counts["branches"].items() if k != "cc_rounds"}
        res["mirror_single_thread_ms"] = {k: round(1e3 * v, 1) for k, v in m.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
