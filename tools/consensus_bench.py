#!/usr/bin/env python3
"""Times the super-read consensus (include/hcsr.h) on one GPU: edge-merge layouts of 150-base single-end reads and cliques
of depth 10 and 40, inside the call (the kernels, by device events) and with the copies (the whole hc_sr_consensus call from
host arrays to host arrays).  Beside it the HOST MIRROR (hc_host_sr_consensus: this project's restatement of
SRBuilder::consensus, not the reference's own loop) on one thread and on 16, on the same box.  Every workload is compared
byte for byte with the mirror before it is timed.  Prints one JSON line per workload.

    python tools/consensus_bench.py [--edges 1000000] [--cliques 100000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import consensus as SR  # noqa: E402
from haploconduct_amd import host, synth  # noqa: E402


def edge_merge_workload(n, seed=1):
    """n merges along edges between overlapping 150-base reads of one genome (true overlaps: the members agree but for read errors)."""
    n_reads = max(2000, n // 8)
    reads, meta = synth.make_single_dataset(n_reads, max(3000, n_reads * 5), flip_frac=0.0, seed=seed)
    cand = synth.single_candidates(meta, min_overlap=60, n_candidates=n, seed=seed + 1)
    e = np.zeros(cand.size, host.EDGE_DTYPE)
    for k in ("read1", "read2", "ori1", "ori2", "pos1"):
        e[k] = cand[k]
    e["v1"], e["v2"] = cand["read1"], cand["read2"]
    layouts, members = host.sr_edge_layouts(e, reads)
    return reads, layouts, members


def clique_workload(n, depth, seed=3):
    """n cliques of `depth` 150-base reads that tile one place of the genome (members start within the first read's length, sorted)."""
    rng = np.random.default_rng(seed)
    n_reads = max(4000, n // 2)
    glen = max(3000, n_reads * 3)
    reads, meta = synth.make_single_dataset(n_reads, glen, flip_frac=0.0, n_strains=1, seed=seed)
    order = np.argsort(meta["s"], kind="stable")
    start = rng.integers(0, n_reads - depth, n)
    idx = order[start[:, None] + np.arange(depth)[None, :]]  # neighbours along the genome
    s = meta["s"][idx]
    pos = s - s[:, :1]
    members = np.zeros(n * depth, SR.SR_MEMBER_DTYPE)
    members["read"], members["pos"] = idx.ravel(), pos.ravel()
    layouts = np.zeros(n, SR.SR_LAYOUT_DTYPE)
    layouts["first_member"], layouts["n_members"] = np.arange(n) * depth, depth
    layouts["total_len"] = (pos + 150).max(axis=1)
    return reads, layouts, members


def best(f, reps):
    out, ts = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return out, min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=1000000)
    ap.add_argument("--cliques", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the mirror's timing (the parity check still runs on 16 threads)")
    a = ap.parse_args()
    work = [("edge_merge", lambda: edge_merge_workload(a.edges), dict(error_correction=False)),
            ("cliques_d10", lambda: clique_workload(a.cliques, 10), dict(error_correction=True, min_clique_size=4)),
            ("cliques_d40", lambda: clique_workload(a.cliques, 40), dict(error_correction=True, min_clique_size=4))]
    with hc.EdgeScorer() as sc:
        for name, make, kw in work:
            reads, layouts, members = make()
            sc.set_reads(reads)
            sc.sr_consensus(layouts[:1000], members, **kw)  # tables, scratch
            dev, t_call = best(lambda: sc.sr_consensus(layouts, members, **kw), a.reps)
            ref, t16 = best(lambda: host.sr_consensus(reads, layouts, members, n_threads=16, **kw), 1 if a.no_host else a.reps)
            same = all(np.array_equal(getattr(dev, k), getattr(ref, k)) for k in ("ret", "status", "out_off", "cons_seq", "cons_qual"))
            t1 = None if a.no_host else best(lambda: host.sr_consensus(reads, layouts, members, n_threads=1, **kw), 1)[1]
            print(json.dumps({"workload": name, "layouts": int(layouts.size), "members": int(members.size), "columns": dev.n_columns,
                              "host_finished_columns": dev.n_host_columns, "host_finished_share": dev.n_host_columns / max(1, dev.n_columns),
                              "device_kernels_ms": round(dev.ms_device, 3), "host_finish_ms": round(dev.ms_host_finish, 3),
                              "device_call_with_copies_ms": round(t_call * 1e3, 3), "mirror_16_threads_ms": round(t16 * 1e3, 3),
                              "mirror_1_thread_ms": None if t1 is None else round(t1 * 1e3, 3), "equal_to_mirror": bool(same),
                              "ok_layouts": int((dev.status == 0).sum())}), flush=True)
            assert same, name + ": the device result differs from the mirror"


if __name__ == "__main__":
    main()
