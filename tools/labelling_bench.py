#!/usr/bin/env python3
"""Times hc_graph_label_vertices and hc_graph_fetch_orientations on the interval graph of tools/graph_clean_bench.py, with the records'
orientations drawn from a random vertex labelling (consistent, many records to switch and to move), and the route a caller had before
the call existed: hc_graph_fetch + the host mirror on one thread + hc_graph_load.  Every device figure is the median of `--reps` runs,
each on a freshly loaded graph (the load is not timed), after one untimed warm-up run; the calls are synchronous, so wall time around
a call is its kernels, its host steps and its read-backs together.

--odd N plants N records against the labelling: the component that holds them becomes inconsistent, its 100 BFS tries run on
`--threads` host threads (n_host_vertices / n_host_edges say how much they read).  --mirror also times the mirror alone, once: with
--odd that is the 100 serial tries the host walk is to be compared with.  Prints one JSON line.

    python tools/labelling_bench.py --vertices 1000000 --degree 22 --mirror
    python tools/labelling_bench.py --vertices 1000000 --degree 22 --odd 10 --threads 16
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import haploconduct_amd as hc  # noqa: E402
from graph_clean_bench import interval_graph, timed  # noqa: E402
from haploconduct_amd.host import HostGraph  # noqa: E402


def orient(edges, V, n_odd, seed):
    """Classes from a hidden labelling; half of the records stand the other way round (to be switched), a third of those turn."""
    rng = np.random.default_rng(seed + 7)
    h = rng.integers(0, 2, V).astype(np.uint8)
    flip = rng.random(edges.size) < 0.5
    o1, o2 = h[edges["v1"].astype(np.int64)], h[edges["v2"].astype(np.int64)]
    edges["ori1"], edges["ori2"] = np.where(flip, 1 - o1, o1), np.where(flip, 1 - o2, o2)
    edges["pos3"] = rng.choice(np.array([-5, 0, 5], np.int32), edges.size)
    if n_odd:
        k = rng.choice(edges.size, n_odd, replace=False)
        edges["ori2"][k] = 1 - edges["ori2"][k]
    return edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--odd", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    edges, out_off, in_nodes, in_off, _, _ = interval_graph(a.vertices, a.degree, a.seed)
    edges = orient(edges, a.vertices, a.odd, a.seed)
    times = dict(label_vertices=[], fetch_orientations=[])
    with hc.EdgeScorer(hc.Settings(n_threads=a.threads)) as sc:
        for rep in range(a.reps + 1):  # the first run warms up (allocations, code objects)
            sc.graph_load(edges, out_off, in_nodes, in_off)
            t0, counts = timed(sc.graph_label_vertices)
            t1, fwd = timed(sc.graph_orientations)
            if rep:
                times["label_vertices"].append(t0), times["fetch_orientations"].append(t1)
        res = dict(vertices=a.vertices, edges=int(edges.size), reps=a.reps, odd=a.odd, threads=a.threads, counts=counts,
                   device_ms={k: round(1e3 * statistics.median(v), 3) for k, v in times.items()},
                   device_ms_min_max={k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in times.items()})
        if a.mirror:  # the route without the call: fetch, the mirror on one thread, load
            sc.graph_load(edges, out_off, in_nodes, in_off)
            t_fetch, f = timed(sc.graph_fetch)
            g = HostGraph(a.vertices, hc.Settings())
            assert g.adopt(f["edges"], f["out_off"], f["in_nodes"], f["in_off"]) == 0
            t_mirror, (m_fwd, m_counts) = timed(g.label_vertices)
            m_edges, _, _ = g.get()
            m_in_off, m_in = g.in_lists(m_edges.shape[0])
            m_out_off = np.concatenate([[0], np.cumsum(np.bincount(m_edges["v1"].astype(np.int64), minlength=a.vertices))]).astype(np.uint64)
            t_load, _ = timed(lambda: sc.graph_load(m_edges, m_out_off, m_in.astype(np.uint32), m_in_off))
            assert np.array_equal(m_fwd, fwd) and all(m_counts[k] == counts[k] for k in ("edges_after", "n_moved", "n_switched", "conflict_count", "best_try"))
            res["host_route_ms"] = dict(fetch=round(1e3 * t_fetch, 1), mirror_single_thread=round(1e3 * t_mirror, 1), load=round(1e3 * t_load, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
