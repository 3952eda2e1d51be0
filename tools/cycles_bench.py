#!/usr/bin/env python3
"""Times hc_graph_sort_edges and hc_graph_remove_cycles on what hc_graph_remove_inclusions, hc_graph_remove_transitive and
hc_graph_remove_tips leave of the interval graph of tools/graph_clean_bench.py (one weak component of nearly every vertex;
--remove-branches runs hc_graph_remove_branches as well, which cuts it into short paths), and the route a caller had before the calls existed: hc_graph_fetch, the host's sortEdges and the mirror
(hc_host_graph_remove_cycles) on one thread, hc_graph_load.  Three cases:

    acyclic   the cleaned graph as it is: one try
    rings     the same graph with `--rings` ring components of `--ring-len` vertices added: 20 tries on a small compact CSR
    giant     the same graph with `--back` records of its largest weak component doubled the other way round: 20 tries on that component

Every device figure is the median of `--reps` runs, each on a freshly loaded graph (the load is not timed), after one untimed warm-up
run; the calls are synchronous, so wall time around a call is its kernels, its host steps and its copies together.  The split of
hc_graph_remove_cycles is the call's own (hc_cycles_counts.ms_*).  The host route is timed once.  Prints one JSON line per case.

    python tools/cycles_bench.py --vertices 1000000 --degree 22 --threads 16
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import haploconduct_amd as hc  # noqa: E402
from graph_clean_bench import interval_graph, timed  # noqa: E402
from haploconduct_amd import cycles as CY  # noqa: E402
from haploconduct_amd.host import EDGE_DTYPE, HostGraph  # noqa: E402

SPLIT = ("ms_first_device", "ms_first_walk", "ms_sub_device", "ms_sub_walk", "ms_edit")


def csr(recs, V):
    """(records, out_off, in_nodes, in_off) with the records grouped by source in the given order."""
    v1, v2 = recs["v1"].astype(np.int64), recs["v2"].astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(np.bincount(v1, minlength=V))]).astype(np.uint64)
    in_off = np.concatenate([[0], np.cumsum(np.bincount(v2, minlength=V))]).astype(np.uint64)
    return recs[np.argsort(v1, kind="stable")], out_off, recs["v1"][np.argsort(v2, kind="stable")].astype(np.uint32), in_off


def weak_components(v1, v2, V):
    """The least vertex of every vertex's weak component: hook the larger label under the smaller, compress, until nothing moves."""
    parent = np.arange(V, dtype=np.int64)
    while True:
        a, b = parent[v1], parent[v2]
        m = a != b
        if not m.any():
            return parent
        np.minimum.at(parent, np.maximum(a, b)[m], np.minimum(a, b)[m])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp


def extra_records(v1, v2, seed):
    rng = np.random.default_rng(seed)
    e = np.zeros(len(v1), EDGE_DTYPE)
    e["v1"], e["v2"], e["read1"], e["read2"] = v1, v2, v1, v2
    e["score"], e["perc"], e["ori1"], e["ori2"], e["ord"] = 1.0, 100, 1, 1, ord("-")
    e["len1"] = e["len0"] = rng.integers(20, 240, len(v1))
    e["pos1"] = 250 - e["len1"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rings", type=int, default=10)
    ap.add_argument("--ring-len", type=int, default=50)
    ap.add_argument("--back", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", default="acyclic,rings,giant")
    ap.add_argument("--remove-branches", action="store_true")
    a = ap.parse_args()
    edges, out_off, in_nodes, in_off, incl, geom = interval_graph(a.vertices, a.degree, a.seed)
    V = a.vertices
    with hc.EdgeScorer(hc.Settings(n_threads=a.threads)) as sc:
        sc.graph_load(edges, out_off, in_nodes, in_off, incl)
        sc.graph_remove_inclusions(), sc.graph_remove_transitive(1, False), sc.graph_remove_tips(150, geom)
        if a.remove_branches:
            sc.graph_remove_branches()
        base = sc.graph_fetch()["edges"]
        del edges, in_nodes
        for case in a.cases.split(","):
            recs, n_v = base, V
            if case == "rings":
                k = np.arange(a.rings * a.ring_len)
                recs = np.concatenate([base, extra_records(V + k, V + (k // a.ring_len) * a.ring_len + (k + 1) % a.ring_len, a.seed)])
                n_v = V + k.size
            elif case == "giant":
                comp = weak_components(base["v1"].astype(np.int64), base["v2"].astype(np.int64), V)
                giant = np.bincount(comp, minlength=V).argmax()
                inside = np.flatnonzero(comp[base["v1"].astype(np.int64)] == giant)
                pick = np.random.default_rng(a.seed + 3).choice(inside, min(a.back, inside.size), replace=False)
                recs = np.concatenate([base, extra_records(base["v2"][pick], base["v1"][pick], a.seed)])
            g = csr(recs, n_v)
            lens = np.full(n_v, 250, np.uint32)
            times = dict(sort_edges=[], remove_cycles=[])
            split = {k: [] for k in SPLIT}
            for rep in range(a.reps + 1):  # the first run warms up (allocations, code objects)
                sc.graph_load(*g)
                t0, sorted_counts = timed(lambda: sc.graph_sort_edges(lens))
                t1, r = timed(lambda: sc.graph_remove_cycles(True))
                if rep:
                    times["sort_edges"].append(t0), times["remove_cycles"].append(t1)
                    for k in SPLIT:
                        split[k].append(r.counts[k])
            after = sc.graph_fetch()
            counts = {k: v for k, v in r.counts.items() if k not in SPLIT}
            res = dict(case=case, branches_removed=a.remove_branches, vertices=n_v, edges=int(recs.size), reps=a.reps, threads=a.threads, sort_counts=sorted_counts, counts=counts,
                       device_ms={k: round(1e3 * statistics.median(v), 3) for k, v in times.items()},
                       device_ms_min_max={k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in times.items()},
                       remove_cycles_split_ms={k[3:]: round(statistics.median(v), 3) for k, v in split.items()})
            # the route without the calls: fetch, the host's sortEdges and the mirror on one thread, load
            sc.graph_load(*g)
            t_fetch, f = timed(sc.graph_fetch)

            def host_steps():
                hg = HostGraph(n_v, hc.Settings())
                assert hg.adopt(f["edges"], f["out_off"], f["in_nodes"], f["in_off"]) == 0
                hg.sort_edges(lens)
                e, _, _ = hg.get()
                i_off, i_nodes = hg.in_lists(e.shape[0])
                o_off = np.concatenate([[0], np.cumsum(np.bincount(e["v1"].astype(np.int64), minlength=n_v))]).astype(np.uint64)
                return CY.host_remove_cycles(e, o_off, i_nodes.astype(np.uint32), i_off, True, 1, cap_pairs=1 << 16)

            t_host, m = timed(host_steps)
            t_load, _ = timed(lambda: sc.graph_load(m.edges, m.out_off, m.in_nodes, m.in_off))
            assert m.pairs.tolist() == r.pairs.tolist() and all(m.counts[k] == r.counts[k] for k in ("edges_after", "backedge_count", "best_try", "try_size"))
            assert np.array_equal(after["edges"]["pos4"], m.edges["pos4"]) and np.array_equal(after["in_nodes"], m.in_nodes)
            res["host_route_ms"] = dict(fetch=round(1e3 * t_fetch, 1), sort_and_mirror_single_thread=round(1e3 * t_host, 1), load=round(1e3 * t_load, 1),
                                        total=round(1e3 * (t_fetch + t_host + t_load), 1))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
