#!/usr/bin/env python3
"""Times hc_br_evidence and hc_br_evidence_fetch on one GPU against the route a caller has without them: hc_graph_fetch +
hc_sr_originals_fetch + hc_host_br_evidence (the mirror) on one thread and on 16.

Workload: --vertices vertices with --branches branches of 2 to 4 neighbours — disjoint fans, half of them out-branches, half in-branches —
over --contig-base contigs; a fan's contigs are one of 64 random sequences with a handful of substitutions per neighbour, so that pairs
differ at a few positions; every contig of a fan holds the same --dict originals of 100 bases cut from its sequence (a tenth of them with
one base changed, half of them listed as reverse), so every entry of a neighbour's dict is common with node1's and the item kernel compares
bases for every one.  Two inputs: dicts of --dict-small and of --dict-large.  The two routes alternate in one process; medians of --reps.
The first device repetition checks every table against the mirror and is not timed.  One JSON line per input (profiles/branch_evidence.md
is those lines' figures), with the imbalance of the item kernel's waves: per wave of 64 consecutive items the largest and the mean number of
covered diff positions a lane walks (computed on the host from the tables).

    python tools/branch_evidence_bench.py [--vertices 100000] [--branches 20000] [--dict-small 50] [--dict-large 1000] [--reps 5] [--host-reps 5]
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
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import branch_evidence as BR  # noqa: E402
from haploconduct_amd import host  # noqa: E402
from haploconduct_amd.originals import ORIGINAL_DTYPE  # noqa: E402
from haploconduct_amd.readstore import ReadSet  # noqa: E402

N_GENOMES, ORIG_LEN = 64, 100
COMP = np.zeros(256, np.uint8)
COMP[:] = np.arange(256)
for a, b in zip(b"ACGT", b"TGCA"):
    COMP[a] = b


def workload(n_vertices, n_branches, contig, dict_size, seed=1):
    rng = np.random.default_rng(seed)
    k = rng.integers(2, 5, n_branches)
    first = np.concatenate([[0], np.cumsum(k + 1)])  # fan b owns the vertices first[b] (node1) .. first[b] + k[b]
    assert first[-1] <= n_vertices, "more fan vertices than vertices"
    genomes = rng.choice(np.frombuffer(b"ACGT", np.uint8), (N_GENOMES, contig))
    genome_of = rng.integers(0, N_GENOMES, n_branches)
    out_side = np.arange(n_branches) % 2 == 0
    V = n_vertices
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), (V, contig))
    member_fan = np.repeat(np.arange(n_branches), k + 1)
    n_mem = member_fan.size
    bases[:n_mem] = genomes[genome_of[member_fan]]
    is_nb = np.ones(n_mem, bool)
    is_nb[first[:-1]] = False
    nb = np.flatnonzero(is_nb)
    for _ in range(6):  # a handful of substitutions per neighbour
        p = rng.integers(0, contig, nb.size)
        bases[nb, p] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, nb.size)]
    reads = ReadSet(bases.reshape(-1), np.full(V * contig, ord("I"), np.uint8), (np.arange(V + 1) * contig).astype(np.uint64),
                    np.arange(V + 1, dtype=np.uint32), np.arange(V, dtype=np.uint64))
    # edges: node1 -> neighbour (out) or neighbour -> node1 (in), all at pos1 0: every pair compares the whole contig
    node1 = first[:-1][member_fan[nb]]
    src = np.where(out_side[member_fan[nb]], node1, nb)
    dst = np.where(out_side[member_fan[nb]], nb, node1)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    edges = np.zeros(src.size, host.EDGE_DTYPE)
    edges["score"], edges["ori1"], edges["ori2"], edges["ord"] = 0.99, 1, 1, ord("-")
    edges["read1"], edges["read2"], edges["v1"], edges["v2"] = src, dst, src, dst
    edges["perc"], edges["len0"], edges["len1"] = 100, contig, contig
    out_off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.uint64)
    io = np.lexsort((src, dst))
    in_nodes = src[io].astype(np.uint32)
    in_off = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=V))]).astype(np.uint64)
    graph = dict(edges=edges, out_off=out_off, in_nodes=in_nodes, in_off=in_off)
    # originals: genome g owns the ids [g * D, (g + 1) * D), cut from it at random offsets
    D = dict_size
    n_orig = N_GENOMES * D
    at = rng.integers(0, contig - ORIG_LEN + 1, n_orig)
    ob = genomes[np.repeat(np.arange(N_GENOMES), D)[:, None], at[:, None] + np.arange(ORIG_LEN)[None, :]].copy()
    changed = np.flatnonzero(rng.random(n_orig) < 0.1)
    ob[changed, rng.integers(0, ORIG_LEN, changed.size)] = ord("N")
    fwd = rng.random(n_orig) < 0.5
    ob[~fwd] = COMP[ob[~fwd][:, ::-1]]
    orig_bases, orig_off = ob.reshape(-1), (np.arange(n_orig + 1) * ORIG_LEN).astype(np.uint64)
    # every fan member's dict is its genome's originals
    sizes = np.zeros(V, np.uint64)
    sizes[:n_mem] = D
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    entries = np.zeros(n_mem * D, ORIGINAL_DTYPE)
    ids = (genome_of[member_fan][:, None] * D + np.arange(D)[None, :]).reshape(-1)
    entries["id"], entries["index1"], entries["len1"], entries["forward"] = ids, at[ids], ORIG_LEN, fwd[ids]
    st = BR.settings(n_orig, 0, n_orig, 50, 0.97)
    return graph, reads, off, entries, orig_bases, orig_off, np.arange(V, dtype=np.uint32), np.ones(V, np.uint8), st


def imbalance(res, graph, off, entries, contig):
    """per wave of 64 consecutive items: the covered diff positions its lanes walk (all contigs start at 0 and every original lies inside
    them, so an item's covered range is the diff positions inside [index1, index1 + 100))"""
    work = []
    for b, r in enumerate(res.branches):
        d = res.diffs(b)
        node, side = int(r["node"]), int(r["side"])
        if side:
            nbs = graph["edges"]["v2"][int(graph["out_off"][node]):int(graph["out_off"][node + 1])]
        else:
            nbs = np.sort(graph["in_nodes"][int(graph["in_off"][node]):int(graph["in_off"][node + 1])])
        for v in nbs:
            i1 = entries["index1"][int(off[int(v)]):int(off[int(v) + 1])]
            work.append(np.searchsorted(d, i1 + ORIG_LEN) - np.searchsorted(d, i1))
        if len(work) > 4000:  # a sample of the branches is enough
            break
    w = np.concatenate(work)
    w = w[:w.size // 64 * 64].reshape(-1, 64)
    return dict(waves=int(w.shape[0]), mean_of_wave_max=round(float(w.max(1).mean()), 2), mean=round(float(w.mean()), 2),
                max=int(w.max()), ratio_max_to_mean=round(float(w.max(1).mean() / max(w.mean(), 1e-9)), 2))


def run(name, w, contig, reps, host_reps):
    graph, reads, off, entries, ob, oo, vread, vfwd, st = w
    dev, fetch_ms, route = [], [], {1: [], 16: []}
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(reads)
        sc.sr_originals_load(off, entries)
        sc.br_set_original_reads(ob, oo)
        res = cn = None
        for rep in range(reps + 1):
            sc.graph_load(graph["edges"], graph["out_off"], graph["in_nodes"], graph["in_off"])
            t0 = time.perf_counter()
            counts = sc.br_evidence(vread, vfwd, st)
            t1 = time.perf_counter()
            res = sc.br_evidence_fetch()
            t2 = time.perf_counter()
            if rep == 0:
                cn = sc._br_counts
                mirror = host.br_evidence(graph, reads, off, entries, ob, oo, vread, vfwd, st, n_threads=16)
                for k in ("branches", "branch_nb", "diff_pos", "ev_edge", "ev_off", "ev_ids", "missing_edges"):
                    assert getattr(res, k).tobytes() == getattr(mirror, k).tobytes(), k
                continue
            dev.append(((t1 - t0) * 1e3, counts["ms_device"]))
            fetch_ms.append((t2 - t1) * 1e3)
            if rep <= host_reps:  # the two routes alternate
                for nt in (1, 16):
                    t0 = time.perf_counter()
                    g = sc.graph_fetch()
                    t1 = time.perf_counter()
                    o, e = sc.sr_originals_fetch()
                    t2 = time.perf_counter()
                    BR.host_evidence(g, reads, o, e, ob, oo, vread, vfwd, st, n_threads=nt, counts=cn)
                    t3 = time.perf_counter()
                    route[nt].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    med = statistics.median

    def cols(r):
        return [round(med(c), 3) for c in zip(*r)]

    c = res.counts
    return {"input": name, "vertices": int(vread.size), "edges": int(graph["edges"].size), "dict_entries": int(entries.size),
            "counts": {k: int(v) for k, v in c.items() if k != "ms_device"}, "reps": reps, "host_reps": len(route[1]),
            "hc_br_evidence_ms[whole call, kernels+sorts+sums (events)]": cols(dev), "whole_call_ms_each": [round(r[0], 3) for r in dev],
            "events_ms_each": [round(r[1], 3) for r in dev], "hc_br_evidence_fetch_ms": round(med(fetch_ms), 3),
            "host_route_1_thread_ms[graph_fetch, originals_fetch, hc_host_br_evidence]": cols(route[1]),
            "host_route_16_threads_ms[graph_fetch, originals_fetch, hc_host_br_evidence]": cols(route[16]),
            "mirror_1_thread_ms_each": [round(r[2], 1) for r in route[1]], "item_wave_imbalance": imbalance(res, graph, off, entries, contig),
            "version": hc.version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--branches", type=int, default=20000)
    ap.add_argument("--contig", type=int, default=1000)
    ap.add_argument("--dict-small", type=int, default=50)
    ap.add_argument("--dict-large", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--only", type=int, help="run input 0 or 1 alone")
    a = ap.parse_args()
    todo = [(f"dicts of {d}", d) for d in (a.dict_small, a.dict_large)]
    for name, d in todo if a.only is None else todo[a.only:a.only + 1]:
        print(json.dumps(run(name, workload(a.vertices, a.branches, a.contig, d), a.contig, a.reps, a.host_reps)), flush=True)


if __name__ == "__main__":
    main()
