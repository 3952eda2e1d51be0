#!/usr/bin/env python3
"""Times hc_sr_merge_next on one GPU on tools/edge_merge_bench.py's path graph: --pairs merges over 150-base reads, as single-end reads and
as 2 x 150 paired reads.  Every repetition starts from the same state (hc_set_reads, then hc_sr_edge_merge with keeping on; neither is timed).

  new call      hc_sr_merge_next whole by wall clock; of it its own kernels and scans (events), the gather and the histograms (events), the
                self-overlap run's kernels (events) and host share, the host's planning, waiting for the copies; the rest is the host's
  parent route  what a caller had before the call, from the same state: numpy glue over the statuses and out_off the edge merge returned,
                hc_sr_merge_self_overlaps_kept on the paired super-reads, the N-rate pre-pass it needs to know which vertices are visited
                (over the consensus bytes the edge merge returned to the host and, for the merged reads, hc_sr_kept_fetch), the entry list,
                hc_sr_set_next_reads.  The route builds no find-next-overlaps tables; the new call does.

The first repetition warms the context and checks the two routes' stores against each other.  Medians of --reps; one JSON line per read type,
and with --markdown the table of profiles/merge_next.md.

    python tools/merge_next_bench.py [--pairs 1000000] [--reps 5] [--markdown profiles/merge_next.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import consensus as SR  # noqa: E402
from haploconduct_amd import next_reads as NR  # noqa: E402
from edge_merge_bench import workload  # noqa: E402


def _n_before(seq):
    c = np.zeros(seq.size + 1, np.int64)
    np.cumsum(seq == ord("N"), out=c[1:])
    return c


def parent_route(sc, reads, pairs, edge, vread, vfwd, keep_singletons):
    """-> (new raw ReadSet's n_reads, the times of its parts in ms)"""
    t0 = time.perf_counter()
    off = edge.result.out_off.astype(np.int64)
    first = edge.first_layout.astype(np.int64)
    nl = first[1:] - first[:-1]
    ok = edge.pair_status == 0
    lens = np.where(edge.result.status == 0, off[1:] - off[:-1], 0)
    l0 = np.minimum(first[:-1], max(lens.size - 1, 0))
    l1 = np.minimum(l0 + 1, max(lens.size - 1, 0))
    len1, len2 = lens[l0], np.where(nl == 2, lens[l1], 0)
    is_pair = ok & (nl == 2)
    cand = np.flatnonzero(is_pair & (len1 > 0) & (len2 > 0))
    sp = np.zeros(cand.size, SR.SR_PAIR_DTYPE)
    sp["off1"], sp["off2"], sp["len1"], sp["len2"] = off[l0[cand]], off[l1[cand]], len1[cand], len2[cand]
    t1 = time.perf_counter()
    m = sc.sr_merge_self_overlaps_kept(sp) if cand.size else None
    t2 = time.perf_counter()
    # the N-rate pre-pass: without it the caller does not know which super-reads survive, hence not which vertices are trivials
    nb = _n_before(edge.result.cons_seq)
    n_count = (nb[off[l0] + len1] - nb[off[l0]]) + np.where(nl == 2, nb[off[l1] + len2] - nb[off[l1]], 0)
    total = len1 + len2
    merged = np.zeros(pairs.shape[0], bool)
    m_off, m_len = np.zeros(pairs.shape[0], np.int64), np.zeros(pairs.shape[0], np.int64)
    if m is not None and m.n_merged:
        hit = m.status == SR.SR_SELF_MERGED
        merged[cand[hit]] = True
        mo = m.out_off.astype(np.int64)
        m_off[cand[hit]], m_len[cand[hit]] = mo[:-1][hit], (mo[1:] - mo[:-1])[hit]
        ms, _ = sc.sr_kept_fetch(int(mo[0]), int(mo[-1] - mo[0]))  # the merged reads' bytes, for their N count
        mb = _n_before(ms)
        n_count[cand[hit]] = mb[mo[1:][hit] - mo[0]] - mb[mo[:-1][hit] - mo[0]]
        total[cand[hit]] = m_len[cand[hit]]
    empty = (len1 == 0) | ((nl == 2) & (len2 == 0))
    alive = ok & ~empty & (n_count.astype(np.float64) < 0.05 * total.astype(np.float64))
    visited = np.zeros(vread.size, bool)
    visited[pairs[alive].reshape(-1)] = True
    # the trivials: short, N rate (the caller holds the reads)
    v = np.flatnonzero(~visited)
    rf = reads.read_first_seq.astype(np.int64)
    so = reads.seq_off.astype(np.int64)
    r = vread[v].astype(np.int64)
    rlen = so[rf[r + 1]] - so[rf[r]]
    rb = _n_before(reads.bases) if v.size else None
    rn = rb[so[rf[r + 1]]] - rb[so[rf[r]]] if v.size else np.zeros(0, np.int64)
    tv = v[(rlen >= keep_singletons) & (rn.astype(np.float64) < 0.05 * rlen.astype(np.float64))]
    single = alive & ((nl == 1) | merged)
    paired = alive & (nl == 2) & ~merged
    e = np.zeros(int(single.sum()) + tv.size + int(paired.sum()), NR.NEXT_ENTRY_DTYPE)
    s_idx, p_idx = np.flatnonzero(single), np.flatnonzero(paired)
    a = e[:s_idx.size]
    a["off1"] = np.where(merged[s_idx], m_off[s_idx], off[l0[s_idx]])
    a["len1"] = np.where(merged[s_idx], m_len[s_idx], len1[s_idx])
    a["kind"] = NR.NEXT_SINGLE
    b = e[s_idx.size:s_idx.size + tv.size]
    b["read"] = vread[tv]
    b["kind"] = np.where(rf[vread[tv].astype(np.int64) + 1] - rf[vread[tv].astype(np.int64)] == 2, NR.NEXT_TRIVIAL_PAIRED, NR.NEXT_TRIVIAL)
    b["rev"] = vfwd[tv] == 0
    c = e[s_idx.size + tv.size:]
    c["off1"], c["len1"], c["off2"], c["len2"], c["kind"] = off[l0[p_idx]], len1[p_idx], off[l1[p_idx]], len2[p_idx], NR.NEXT_PAIRED
    t3 = time.perf_counter()
    res = sc.sr_set_next_reads(e, keep_singletons=keep_singletons)
    t4 = time.perf_counter()
    assert (res.status == NR.NEXT_KEPT).all()
    return e.size, ((t1 - t0 + t3 - t2) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, (t4 - t0) * 1e3)


def run(n_pairs, paired, reps, keep_singletons=0):
    reads, graph, vread, vfwd = workload(n_pairs, paired)
    cap = n_pairs * (2 if paired else 1) * 340
    rows = {"new": [], "parent": []}
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        sc.graph_load(*graph)
        pairs = sc.graph_merge_pairs()
        for rep in range(reps + 1):
            stores = []
            for route in ("new", "parent"):
                sc.set_reads(reads)
                edge = sc.sr_edge_merge(pairs, vread, vfwd, cap=cap)
                if route == "new":
                    t0 = time.perf_counter()
                    res = sc.sr_merge_next(pairs, edge, vread, vfwd, keep_singletons=keep_singletons)
                    whole = (time.perf_counter() - t0) * 1e3
                    dev = res.ms_device + res.counts["ms_device"] + res.self_stats["ms_device"]
                    row = (whole, res.ms_device, res.counts["ms_device"], res.self_stats["ms_device"], res.self_stats["ms_host"], res.counts["ms_plan"],
                           res.ms_copy, whole - dev - res.self_stats["ms_host"] - res.counts["ms_plan"] - res.ms_copy)
                    n_new = res.new_read_count
                else:
                    n_new, row = parent_route(sc, reads, pairs, edge, vread, vfwd, keep_singletons)
                if rep == 0:
                    stores.append((n_new, sc.sr_next_reads_fetch()))
                else:
                    rows[route].append(row)
            if rep == 0:
                (na, a), (nb, b) = stores
                assert na == nb and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("bases", "quals", "seq_off", "read_first_seq"))
    med = statistics.median

    def cols(r):
        return [round(med(c), 3) for c in zip(*r)]

    return {"workload": "path, " + ("2 x 150 paired" if paired else "150 single-end"), "pairs": n_pairs, "vertices": int(vread.size), "reps": reps,
            "new_reads": int(res.new_read_count), "singles": res.n_singles, "trivials": res.n_trivials, "paired": res.n_paired,
            "self_merged": res.n_self_merged, "self_host_pairs": int(res.self_stats["n_host_pairs"]),
            "merge_next_ms[whole, own kernels, gather+hist, self kernels, self host, plan, copies, other host]": cols(rows["new"]),
            "parent_route_ms[numpy glue, self_overlaps_kept, set_next_reads, whole]": cols(rows["parent"]), "version": hc.version()}


def markdown(results, commit):
    s, p = results
    nk, pk = "merge_next_ms[whole, own kernels, gather+hist, self kernels, self host, plan, copies, other host]", \
        "parent_route_ms[numpy glue, self_overlaps_kept, set_next_reads, whole]"
    names = ["**`hc_sr_merge_next`, whole call**", "— its own kernels and scans (events)", "— gather and histograms (events)", "— self-overlap kernels (events)",
             "— self-overlap host share (tables, host-decided pairs)", "— planning (`plan_store`)", "— waiting for the copies of inputs and tables",
             "— other host (pair list, encoder launch, allocation)"]
    lines = [f"Parent commit of the change that added the call: `{commit}`.  ms, medians of {s['reps']}, one MI355X.", "",
             "| part | single-end | 2 x 150 paired |", "|---|---|---|",
             f"| pairs / vertices | {s['pairs']} / {s['vertices']} | {p['pairs']} / {p['vertices']} |",
             f"| new store: singles / trivials / pairs | {s['singles']} / {s['trivials']} / {s['paired']} | {p['singles']} / {p['trivials']} / {p['paired']} |",
             f"| self-merged pairs (host-decided) | {s['self_merged']} ({s['self_host_pairs']}) | {p['self_merged']} ({p['self_host_pairs']}) |"]
    lines += [f"| {n} | {s[nk][i]} | {p[nk][i]} |" for i, n in enumerate(names)]
    pn = ["parent route: numpy glue with the N-rate pre-pass", "— `hc_sr_merge_self_overlaps_kept`", "— `hc_sr_set_next_reads`", "**parent route, whole (no FNO tables)**"]
    lines += [f"| {n} | {s[pk][i]} | {p[pk][i]} |" for i, n in enumerate(pn)]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", help="write the figures' table to this file")
    ap.add_argument("--parent-commit", help="hash of the commit the parent route stands for (default: the parent of git's HEAD)")
    a = ap.parse_args()
    results = []
    for paired in (False, True):
        results.append(run(a.pairs, paired, a.reps))
        print(json.dumps(results[-1]), flush=True)
    if a.markdown:
        commit = a.parent_commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD~1"], capture_output=True, text=True).stdout.strip()
        with open(a.markdown, "w") as f:
            f.write(markdown(results, commit or "unknown"))


if __name__ == "__main__":
    main()
