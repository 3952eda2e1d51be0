#!/usr/bin/env python3
"""Times hc_sr_clique_next on one GPU on tools/clique_merge_bench.py's workload: --cliques cliques of 3 to 40 vertices over 150-base reads,
half of them pairs, laid out and merged by hc_sr_clique_merge (not timed here: profiles/clique_merge.md).

  new call      hc_sr_clique_next whole by wall clock; of it its own kernels, sorts and scans (events), the gather and the histograms
                (events), the self-overlap kernels (events) and host share, the store's planning on the host, the waits for the copies of
                the inputs and the tables, and what is left: the host's pass over the cliques, allocation, the encoder's launches
  parent route  what a caller had before this call: hc_sr_kept_fetch of the consensus bytes, the marks, trivials, numbering and tables on
                the host — the mirror hc_host_sr_clique_next stands in for the caller's code —, and hc_set_reads of the next store

The first run warms the context and checks the routes against each other: every output array and the raw arrays of the store.  Medians of
--reps runs; one JSON line, and with --markdown the table of profiles/clique_next.md.

    python tools/clique_next_bench.py [--cliques 20000] [--reps 5] [--markdown profiles/clique_next.md]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import clique_next as CN  # noqa: E402
from haploconduct_amd import host  # noqa: E402
from clique_merge_bench import M, workload  # noqa: E402

KEEP_SINGLETONS = 100


def run(n_cliques, reps):
    reads, graph, off, nodes, vread, vfwd = workload(n_cliques)
    rows, parent = [], []
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        for rep in range(reps + 1):
            sc.set_reads(reads)
            sc.graph_load(*graph)
            merged = sc.sr_clique_merge(off, nodes, vread, vfwd, min_clique_size=M)
            t0 = time.perf_counter()
            dev = sc.sr_clique_next(off, nodes, merged, vread, vfwd, keep_singletons=KEEP_SINGLETONS)
            t1 = time.perf_counter()
            raw = sc.sr_next_reads_fetch() if rep == 0 else None
            # the parent route from the same state: the store and the kept bytes as the clique merge left them
            sc.set_reads(reads)
            sc.sr_kept_load(merged.result.cons_seq, merged.result.cons_qual)
            p0 = time.perf_counter()
            cs, cq = sc.sr_kept_fetch()
            p1 = time.perf_counter()
            ref = host.sr_clique_next(reads, cs, cq, off, nodes, merged, vread, vfwd, keep_singletons=KEEP_SINGLETONS, n_threads=16)
            p2 = time.perf_counter()
            sc.set_reads(ref.reads)
            p3 = time.perf_counter()
            if rep == 0:
                for k in CN.ARRAYS:
                    assert getattr(dev, k).tobytes() == getattr(ref, k).tobytes(), k
                for k in ("read_first_seq", "seq_off", "bases", "quals"):
                    assert np.array_equal(getattr(raw, k), getattr(ref.reads, k)), k
                continue
            whole = (t1 - t0) * 1e3
            parts = [dev.ms_device, dev.counts["ms_device"], dev.self_stats["ms_device"], dev.self_stats["ms_host"], dev.counts["ms_plan"], dev.ms_copy]
            rows.append([whole] + parts + [whole - sum(parts)])
            parent.append(((p1 - p0) * 1e3, (p2 - p1) * 1e3, (p3 - p2) * 1e3, (p3 - p0) * 1e3))
    med = statistics.median
    cols = lambda r: [round(med(c), 3) for c in zip(*r)]  # noqa: E731
    return {"workload": "tools/clique_merge_bench.py's: piles of 150-base reads, half of them pairs, min_clique_size 4", "cliques": n_cliques,
            "clique_entries": int(off[-1]), "vertices": int(vread.size), "members": int(merged.member_vertex.size), "keep_singletons": KEEP_SINGLETONS,
            "super_reads[single, self-merged of them, paired]": [dev.n_singles, dev.n_self_merged, dev.n_paired], "trivials": dev.n_trivials,
            "row_entries": int(dev.clique_nodes.size), "new_reads": dev.new_read_count, "new_bases": dev.counts["n_bytes"], "reps": reps,
            "clique_next_ms[whole, own kernels, gather+hist, self kernels, self host, plan, copies, other host]": cols(rows),
            "parent_route_ms[kept_fetch, mirror, hc_set_reads, whole]": cols(parent), "version": hc.version()}


def markdown(r):
    nk, pk = "clique_next_ms[whole, own kernels, gather+hist, self kernels, self host, plan, copies, other host]", \
        "parent_route_ms[kept_fetch, mirror, hc_set_reads, whole]"
    names = ["**`hc_sr_clique_next`, whole call**", "— its own kernels, sorts and scans (events)", "— gather and histograms (events)",
             "— self-overlap kernels (events)", "— self-overlap, host share", "— the store's planning on the host", "— waiting for the copies of inputs and tables",
             "— the rest on the host (the pass over the cliques, allocation, the encoder's launches)"]
    pnames = ["parent route: `hc_sr_kept_fetch`", "— marks, trivials, numbering, tables on the host (the mirror)", "— `hc_set_reads` of the next store",
              "**parent route, whole**"]
    s = r["super_reads[single, self-merged of them, paired]"]
    lines = ["| part | ms |", "|---|---|",
             f"| cliques / clique entries / vertices / members | {r['cliques']} / {r['clique_entries']} / {r['vertices']} / {r['members']} |",
             f"| super-reads: single (self-merged of them) / paired; trivials | {s[0]} ({s[1]}) / {s[2]}; {r['trivials']} |",
             f"| row entries / reads and bases of the next store | {r['row_entries']} / {r['new_reads']}, {r['new_bases']} |"]
    lines += [f"| {n} | {v} |" for n, v in zip(names, r[nk])]
    lines += [f"| {n} | {v} |" for n, v in zip(pnames, r[pk])]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cliques", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", help="write the figures' table here (the text around it in profiles/clique_next.md is written by hand)")
    a = ap.parse_args()
    r = run(a.cliques, a.reps)
    print(json.dumps(r), flush=True)
    if a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        with open(a.markdown, "w") as f:
            f.write(markdown(r))


if __name__ == "__main__":
    main()
