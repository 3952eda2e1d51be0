#!/usr/bin/env python3
"""Times hc_graph_cliques and hc_graph_cliques_fetch against the host mirror hc_host_graph_cliques (1 and 16 threads) on an
interval-like graph: read i -> reads i + 1 .. i + degree / 2 (mean degree about `--degree`), a fraction `--knock-out` of the records
left out, inserted in a random order.  Every figure is the median of `--reps` runs after one untimed warm-up: ms_device (the call's
kernels, sorts and scans by events — kernel time apart from copies), ms_host (the host-route roots), the whole call (wall), the fetch
of the CSR (wall), and the mirror's wall time.  The budget (`--max-entries`) applies to all of them: a perturbed interval graph can
hold far more cliques than memory.  Prints one JSON line.

    python tools/cliques_bench.py --vertices 100000 --degree 50
    python tools/cliques_bench.py --vertices 20000 --degree 500 --mirror-reps 1
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import cliques as CL  # noqa: E402
from haploconduct_amd.host import EDGE_DTYPE  # noqa: E402


def interval_graph(V, degree, knock_out, seed):
    rng = np.random.default_rng(seed)
    v1, v2 = [], []
    for d in range(1, degree // 2 + 1):
        a = np.arange(V - d, dtype=np.int64)
        ok = rng.random(V - d) >= knock_out
        v1.append(a[ok])
        v2.append(a[ok] + d)
    v1, v2 = np.concatenate(v1), np.concatenate(v2)
    p = rng.permutation(v1.size)
    v1, v2 = v1[p], v2[p]
    e = np.zeros(v1.size, EDGE_DTYPE)
    e["v1"], e["v2"], e["read1"], e["read2"] = v1, v2, v1, v2
    e["score"], e["perc"], e["ori1"], e["ori2"], e["ord"] = 1.0, 100, 1, 1, ord("-")
    order = np.argsort(v1, kind="stable")
    out_off = np.concatenate([[0], np.cumsum(np.bincount(v1, minlength=V))]).astype(np.uint64)
    in_order = np.argsort(v2, kind="stable")
    in_off = np.concatenate([[0], np.cumsum(np.bincount(v2, minlength=V))]).astype(np.uint64)
    return e[order], out_off, v1[in_order].astype(np.uint32), in_off


def median(x):
    return round(statistics.median(x), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--degree", type=int, default=50)
    ap.add_argument("--knock-out", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mirror-reps", type=int, default=5)
    ap.add_argument("--root-cap", type=int, default=0)
    ap.add_argument("--max-entries", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    V = a.vertices
    g = interval_graph(V, a.degree, a.knock_out, a.seed)
    res = dict(vertices=V, records=int(g[0].size), degree=a.degree, knock_out=a.knock_out, reps=a.reps)
    with hc.EdgeScorer(hc.Settings()) as sc:
        sc.graph_load(*g)
        dev, host, call, fetch = [], [], [], []
        got = None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            got = sc.graph_cliques(root_cap=a.root_cap, max_entries=a.max_entries, fetch=False)
            t1 = time.perf_counter()
            c = got.counts
            if c["status"] == 0:
                off, nodes = np.zeros(c["n_cliques"] + 1, np.uint64), np.zeros(max(c["n_entries"], 1), np.uint32)
                t2 = time.perf_counter()
                hc._native.check(hc._native.lib.hc_graph_cliques_fetch(sc._ctx, off.ctypes.data, nodes.ctypes.data), "hc_graph_cliques_fetch")
                t3 = time.perf_counter()
            else:
                t2 = t3 = 0.0
            if rep:
                dev.append(c["ms_device"]), host.append(c["ms_host"]), call.append(1e3 * (t1 - t0)), fetch.append(1e3 * (t3 - t2))
        c = got.counts
        res["device"] = dict(status=CL.CLIQUES_STATUS[c["status"]], n_pairs=c["n_pairs"], n_cliques=c["n_cliques"], n_entries=c["n_entries"],
                             max_clique=c["max_clique"], n_host_roots=c["n_host_roots"], ms_device=median(dev), ms_host=median(host),
                             ms_call=median(call), ms_fetch=median(fetch), ms_device_min_max=[round(min(dev), 3), round(max(dev), 3)])
    for nt in (1, 16):
        t = []
        m = None
        for rep in range(a.mirror_reps + (1 if a.mirror_reps > 1 else 0)):
            t0 = time.perf_counter()
            # one enumeration, into buffers sized by the device's counts (the Python wrapper would count, then fetch)
            st, m = CL.hc_cliques_settings(0, nt, a.max_entries), CL.hc_cliques_counts()
            off, nodes = np.zeros(c["n_cliques"] + 1, np.uint64), np.zeros(max(c["n_entries"], 1), np.uint32)
            t0 = time.perf_counter()
            hc._native.check(hc._native.lib.hc_host_graph_cliques(g[0].ctypes.data, g[1].ctypes.data, V, None, C.byref(st), off.ctypes.data,
                                                                  nodes.ctypes.data, c["n_cliques"], c["n_entries"], C.byref(m)), "hc_host_graph_cliques")
            if rep or a.mirror_reps == 1:
                t.append(1e3 * (time.perf_counter() - t0))
        assert m.status == c["status"] and m.n_cliques == c["n_cliques"] and m.n_entries == c["n_entries"]
        res[f"mirror_{nt}_threads_ms"] = median(t)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
