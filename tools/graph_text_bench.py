#!/usr/bin/env python3
"""Times hc_graph_write_text and hc_graph_text_fetch for the three kinds (graph.txt, digraph.txt, GFA) on the interval graph of
tools/graph_clean_bench.py — as loaded, with a fraction of reverse records added (so that graph.txt's checkEdge look-up has work),
and on what the four cleaning calls leave of it — with 150-base single-end reads for GFA.  Every figure is the median of `--reps`
runs after one untimed warm-up: ms_device (the call's kernels and scans by events), the whole call (wall), and the fetch of the whole
text into host memory (wall).  For comparison: hc_graph_fetch alone on the same graph (80 bytes per edge and the small arrays), a lower
bound for any route that writes the text on the host.  Prints one JSON line.

    python tools/graph_text_bench.py --vertices 1000000 --degree 22
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import _native as N  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402

_spec = importlib.util.spec_from_file_location("graph_clean_bench", os.path.join(ROOT, "tools", "graph_clean_bench.py"))
clean_bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(clean_bench)


def with_reverse(edges, V, frac, seed):
    """The graph with the reverse record of a fraction of its edges inserted behind them (scores above 0: graph.txt skips them)."""
    rng = np.random.default_rng(seed)
    pick = edges[rng.random(edges.size) < frac].copy()
    pick["v1"], pick["v2"] = pick["v2"].copy(), pick["v1"].copy()
    pick["read1"], pick["read2"] = pick["v1"], pick["v2"]
    e = np.concatenate([edges, pick])
    v1, v2 = e["v1"].astype(np.int64), e["v2"].astype(np.int64)
    order = np.argsort(v1, kind="stable")
    out_off = np.concatenate([[0], np.cumsum(np.bincount(v1, minlength=V))]).astype(np.uint64)
    in_order = np.argsort(v2, kind="stable")
    in_off = np.concatenate([[0], np.cumsum(np.bincount(v2, minlength=V))]).astype(np.uint64)
    return e[order], out_off, v1[in_order].astype(np.uint32), in_off


def measure(sc, kinds, n_singles, reps):
    out = {}
    for kind in kinds:
        st = N.hc_graph_text_settings(0.0, 0.0, n_singles)
        c = N.hc_graph_text_counts()
        dev, call, fetch = [], [], []
        buf = np.empty(0, np.uint8)
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            N.check(N.lib.hc_graph_write_text(sc._ctx, N.GRAPH_TEXT_KINDS[kind], C.byref(st), C.byref(c)), "hc_graph_write_text")
            t1 = time.perf_counter()
            assert c.status == 0, (kind, N.GRAPH_TEXT_STATUS[c.status], c.bad_v, c.bad_pos)
            if buf.size < c.n_bytes:
                buf = np.empty(int(c.n_bytes), np.uint8)
                buf[:] = 0  # (touched before it is timed)
            t2 = time.perf_counter()
            N.check(N.lib.hc_graph_text_fetch(sc._ctx, 0, c.n_bytes, buf.ctypes.data), "hc_graph_text_fetch")
            t3 = time.perf_counter()
            if rep:
                dev.append(c.ms_device)
                call.append(1e3 * (t1 - t0))
                fetch.append(1e3 * (t3 - t2))
        out[kind] = dict(n_bytes=int(c.n_bytes), n_lines=int(c.n_lines), ms_device=round(statistics.median(dev), 3),
                         ms_call=round(statistics.median(call), 3), ms_fetch=round(statistics.median(fetch), 3),
                         ms_device_min_max=[round(min(dev), 3), round(max(dev), 3)])
    t = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        sc.graph_fetch()
        if rep:
            t.append(1e3 * (time.perf_counter() - t0))
    out["hc_graph_fetch_ms"] = round(statistics.median(t), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reverse", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    V = a.vertices
    edges, out_off, in_nodes, in_off, incl, geom = clean_bench.interval_graph(V, a.degree, a.seed)
    rng = np.random.default_rng(a.seed + 7)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, V * a.read_len)]
    reads = ReadSet(bases, np.full(bases.size, ord("I"), np.uint8), np.arange(0, bases.size + 1, a.read_len, dtype=np.uint64),
                    np.arange(V + 1, dtype=np.uint32), np.arange(V))
    res = dict(vertices=V, reps=a.reps, read_len=a.read_len)
    with hc.EdgeScorer(hc.Settings()) as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        sc.graph_load(edges, out_off, in_nodes, in_off)
        res["loaded"] = dict(edges=int(edges.size), **measure(sc, ("cliques", "digraph", "gfa"), V, a.reps))
        r = with_reverse(edges, V, a.reverse, a.seed + 3)
        sc.graph_load(*r)
        res["with_reverse"] = dict(edges=int(r[0].size), **measure(sc, ("cliques",), V, a.reps))
        sc.graph_load(edges, out_off, in_nodes, in_off, incl)
        sc.graph_remove_inclusions()
        sc.graph_remove_transitive(1, False)
        sc.graph_remove_tips(150, geom)
        sc.graph_remove_branches()
        res["cleaned"] = dict(edges=sc._graph_size()[1], **measure(sc, ("cliques", "digraph", "gfa"), V, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
