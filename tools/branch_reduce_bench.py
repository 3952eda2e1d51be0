#!/usr/bin/env python3
"""Times hc_br_reduce on one GPU, with its phase split, against the route a caller had before it: hc_br_evidence_fetch + hc_graph_fetch +
hc_host_br_reduce (the mirror, one thread) + hc_graph_load.

Workload: tools/branch_evidence_bench.py's two inputs (--vertices vertices, --branches disjoint fans of 2 to 4 neighbours, dicts of
--dict-small and --dict-large), reduced with a table that gives every dist a min_evidence of --min-evidence, diploid on, careful on.  Both
routes start from the same state: the graph loaded, hc_br_evidence run (neither is timed).  The routes alternate in one process; medians of
--reps.  The first repetition checks the device's tables, graph and branching_edges against the mirror's and is not timed.  One JSON line
per input (profiles/branch_reduce.md is those lines' figures): the whole call by the host's clock, the call's own split — host walk and
chain, the radix sort, the other kernels, the edit, the copies —, the caller's route piece by piece, the components the host finished.

    python tools/branch_reduce_bench.py [--vertices 100000] [--branches 20000] [--dict-small 50] [--dict-large 1000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import branch_evidence as BR  # noqa: E402
from haploconduct_amd import host  # noqa: E402
from branch_evidence_bench import workload  # noqa: E402


def run(name, w, reps, min_evidence):
    graph, reads, off, entries, ob, oo, vread, vfwd, st = w
    settings = BR.reduce_settings({d: min_evidence for d in range(1, 20000)}, careful=True, diploid=True)
    dev, route = [], []
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        sc.sr_originals_load(off, entries)
        sc.br_set_original_reads(ob, oo)
        counts = None
        for rep in range(reps + 1):
            sc.graph_load(graph["edges"], graph["out_off"], graph["in_nodes"], graph["in_off"])
            sc.br_evidence(vread, vfwd, st)
            t0 = time.perf_counter()
            counts = sc.br_reduce(settings)
            t1 = time.perf_counter()
            if rep == 0:
                red, g2, br = sc.br_reduce_fetch(), sc.graph_fetch(), sc.graph_branching_edges()
                sc.graph_load(graph["edges"], graph["out_off"], graph["in_nodes"], graph["in_off"])
                sc.br_evidence(vread, vfwd, st)
                m_red, m_g, m_br = host.br_reduce(sc.graph_fetch(), reads, sc.br_evidence_fetch(), settings)
                for k in ("components", "comp_edge", "comp_unique", "removed"):
                    assert getattr(red, k).tobytes() == getattr(m_red, k).tobytes(), k
                for k in ("edges", "out_off", "in_nodes", "in_off"):
                    assert g2[k].tobytes() == m_g[k].tobytes(), k
                assert br.tobytes() == m_br.tobytes()
                continue
            dev.append(((t1 - t0) * 1e3, counts["ms_host_walk"], counts["ms_sort"], counts["ms_device"] - counts["ms_sort"] - counts["ms_edit"], counts["ms_edit"],
                        counts["ms_copy"]))
            # the caller's route from the same state
            sc.graph_load(graph["edges"], graph["out_off"], graph["in_nodes"], graph["in_off"])
            sc.br_evidence(vread, vfwd, st)
            t0 = time.perf_counter()
            ev = sc.br_evidence_fetch()
            t1 = time.perf_counter()
            g = sc.graph_fetch()
            t2 = time.perf_counter()
            _, mg, _ = host.br_reduce(g, reads, ev, settings)
            t3 = time.perf_counter()
            sc.graph_load(mg["edges"], mg["out_off"], mg["in_nodes"], mg["in_off"])
            t4 = time.perf_counter()
            route.append(((t4 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))
    med = statistics.median

    def cols(r):
        return [round(med(c), 3) for c in zip(*r)]

    return {"input": name, "vertices": int(vread.size), "edges": int(graph["edges"].size),
            "counts": {k: int(v) for k, v in counts.items() if not k.startswith("ms_")}, "reps": reps,
            "hc_br_reduce_ms[whole call, host walk+chain, sort, other kernels, edit, copies]": cols(dev),
            "whole_call_ms_each": [round(r[0], 3) for r in dev],
            "caller_route_ms[whole, evidence_fetch, graph_fetch, hc_host_br_reduce 1 thread, graph_load]": cols(route),
            "route_ms_each": [round(r[0], 1) for r in route],
            "host_finished_share": round(counts["n_host_finished"] / max(counts["n_components"], 1), 4), "version": hc.version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--branches", type=int, default=20000)
    ap.add_argument("--contig", type=int, default=1000)
    ap.add_argument("--dict-small", type=int, default=50)
    ap.add_argument("--dict-large", type=int, default=1000)
    ap.add_argument("--min-evidence", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, help="run input 0 or 1 alone")
    a = ap.parse_args()
    todo = [(f"dicts of {d}", d) for d in (a.dict_small, a.dict_large)]
    for name, d in todo if a.only is None else todo[a.only:a.only + 1]:
        print(json.dumps(run(name, workload(a.vertices, a.branches, a.contig, d), a.reps, a.min_evidence)), flush=True)


if __name__ == "__main__":
    main()
