"""FNO=1 of an edge-merge iteration, two routes on tools/fno_bench.py's workload (10^6 vertices, 2.5 * 10^5 super-reads, 4 * 10^6 edges,
2 * 10^5 branching edges, 2 * 10^6 stored non-edges) loaded as a device graph:
  (old) what a caller had before hc_fno1_from_graph: hc_graph_fetch, hc_graph_fetch_branching_edges, hc_graph_fetch_inclusion_edges,
        fno.edges_from_graph on every record, hc_fno1_run, the text on the host;
  (new) hc_fno1_from_graph with the caller's tables, then hc_fno1_text_fetch; and hc_fno1_lines_device, which fetches nothing.
The routes alternate in one process; medians of --reps runs and the spread (max - min) of each.  The new route counts as faster only where
its median lies below the old one's by more than three times the old route's spread (profiles/fastq_reader.md's rule).  A call with no
super-read, no non-edge and no inclusion group has nothing but the conversion kernel in the second of the call's four timed sections
(hc_fno1_section_ms): `convert_ms` for `conversion_bytes` read and written, `convert_GBps` from the two.  Then tools/merge_next_bench.py's path workload (--pairs pairs) through hc_sr_edge_merge and hc_sr_merge_next:
the call with the tables kept on the device against the same call with the returned host tables.  Prints one JSON line per workload.
  python tools/fno1_resident_bench.py [--nodes 1000000] [--srs 250000] [--edges 4000000] [--pairs 1000000] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import fno as F  # noqa: E402
from haploconduct_amd.host import EDGE_DTYPE  # noqa: E402
from tools.fno_bench import big_fno1  # noqa: E402


def med(xs):
    return round(statistics.median(xs), 3), round(max(xs) - min(xs), 3)


def device_graph(sc, inp):
    """the workload's graph_edges as the device graph (adj_in rebuilt from the out-lists), its branching_edges left out: the device
    keeps those only behind its own cleaning calls"""
    V = len(inp.nodes)
    e = np.zeros(len(inp.graph_edges), EDGE_DTYPE)
    for f in ("v1", "v2", "score", "pos1", "pos2", "len1", "len2", "perc", "ord", "ori1", "ori2"):
        e[f] = inp.graph_edges[f]
    e["read1"], e["read2"] = e["v1"], e["v2"]
    v1, v2 = e["v1"].astype(np.int64), e["v2"].astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(np.bincount(v1, minlength=V))]).astype(np.uint64)
    order = np.argsort(v2, kind="stable")
    in_off = np.concatenate([[0], np.cumsum(np.bincount(v2, minlength=V))]).astype(np.uint64)
    sc.graph_load(e, out_off, e["v1"][order].astype(np.uint32), in_off)


def old_route(sc, tables, nonedges, **kw):
    t0 = time.perf_counter()
    inp = F.input_from_context(sc, tables, nonedges, **kw)  # the three fetches, edges_from_graph
    t1 = time.perf_counter()
    text, cnt = F.find_next_overlaps(inp)
    t2 = time.perf_counter()
    return dict(fetch_convert=(t1 - t0) * 1e3, run=F.last_run_s * 1e3, total=(t2 - t0) * 1e3), text, cnt


def new_route(sc, tables, nonedges, **kw):
    t0 = time.perf_counter()
    res = sc.fno1_from_graph(tables, nonedges, **kw)
    t1 = time.perf_counter()
    text = sc.fno1_text()
    t2 = time.perf_counter()
    p, n = sc.fno1_lines_device()
    t3 = time.perf_counter()
    sec = sc.fno1_section_ms()
    return dict(call=(t1 - t0) * 1e3, ms_device=res.counts["ms_device"], ms_pairs=sec[0], ms_build=sec[1], ms_segments34=sec[2], ms_walk=sec[3], text_fetch=(t2 - t1) * 1e3, lines_device=(t3 - t2) * 1e3,
                total=(t2 - t0) * 1e3, total_lines_only=(t1 - t0 + t3 - t2) * 1e3), text, res.counts


def verdict(res, old_key, new_key):
    (o, o_spread), (n, _) = res[old_key]["total"], res[new_key]["total"]
    res["faster_by_the_three_spreads_rule"] = bool(o - n > 3 * o_spread)
    res["old_over_new"] = round(o / n, 2) if n else None


def fno_workload(a):
    inp = big_fno1(a.nodes, a.srs, a.edges)
    tables = (inp.nodes, inp.srs, inp.clique_off, inp.clique_nodes, inp.subread_off, inp.subreads, inp.new_read_count)
    res = {"workload": "tools/fno_bench.py big_fno1", "vertices": a.nodes, "super_reads": a.srs, "graph_edges": a.edges, "nonedges": len(inp.nonedges),
           "reps": a.reps, "version": hc.version()}
    with hc.EdgeScorer() as sc:
        device_graph(sc, inp)
        old_route(sc, tables, inp.nonedges), new_route(sc, tables, inp.nonedges)  # warm: allocations, the first launches
        to, tn = [], []
        for _ in range(a.reps):
            x, text_o, cnt_o = old_route(sc, tables, inp.nonedges)
            y, text_n, cnt_n = new_route(sc, tables, inp.nonedges)
            to.append(x), tn.append(y)
        res["same_text"] = bool(text_o == text_n)
        res["old_route_ms"] = {k: med([t[k] for t in to]) for k in to[0]}
        res["new_route_ms"] = {k: med([t[k] for t in tn]) for k in tn[0]}
        res["old_route_device_level"] = F.last_device_level
        res.update(n_lines=cnt_n["n_lines"], n_bytes=cnt_n["n_bytes"], n_items=cnt_n["n_items"], n_nonedges_kept=cnt_n["n_nonedges_kept"])
        verdict(res, "old_route_ms", "new_route_ms")
        # the conversion alone: with no super-read, no non-edge and no inclusion group, section 1 of the call (hc_fno1_section_ms) holds the
        # conversion kernel and two memsets' worth of nothing else
        empty = (inp.nodes, inp.srs[:0], np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint64), inp.subreads[:0], inp.new_read_count)
        sc.fno1_from_graph(empty)
        ms = []
        for _ in range(a.reps):
            sc.fno1_from_graph(empty)
            ms.append(sc.fno1_section_ms()[1])
        res["convert_ms"] = med(ms)
        res["conversion_bytes"] = a.edges * (80 + 48)
        res["convert_GBps"] = round(res["conversion_bytes"] / (res["convert_ms"][0] * 1e-3) / 1e9, 1) if res["convert_ms"][0] else None
    return res


def kept_workload(a):
    from tools.edge_merge_bench import workload

    reads, graph, vread, vfwd = workload(a.pairs, False)
    res = {"workload": "tools/merge_next_bench.py path, 150 single-end", "pairs": a.pairs, "vertices": int(vread.size), "reps": a.reps}
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        sc.graph_load(*graph)
        pairs = sc.graph_merge_pairs()
        edge = sc.sr_edge_merge(pairs, vread, vfwd, cap=a.pairs * 340)
        dev = sc.sr_merge_next(pairs, edge, vread, vfwd)
        new_route(sc, None, None), new_route(sc, dev, None), old_route(sc, dev, None)
        tk, tc, to = [], [], []
        for _ in range(a.reps):
            x, text_k, _ = new_route(sc, None, None)
            y, text_c, _ = new_route(sc, dev, None)
            z, text_o, _ = old_route(sc, dev, None)
            tk.append(x), tc.append(y), to.append(z)
        res["same_text"] = bool(text_k == text_c == text_o)
        res["kept_tables_ms"] = {k: med([t[k] for t in tk]) for k in tk[0]}
        res["caller_tables_ms"] = {k: med([t[k] for t in tc]) for k in tc[0]}
        res["old_route_ms"] = {k: med([t[k] for t in to]) for k in to[0]}
        res["n_lines"] = int(text_k.count(b"\n"))
        verdict(res, "old_route_ms", "kept_tables_ms")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--srs", type=int, default=250_000)
    ap.add_argument("--edges", type=int, default=4_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(fno_workload(a)), flush=True)
    if a.pairs:
        print(json.dumps(kept_workload(a)), flush=True)


if __name__ == "__main__":
    main()
