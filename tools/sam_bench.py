#!/usr/bin/env python3
"""The SAM ingest's enumeration on the device (hc_sam_plan + every line range, lines kept in device memory) beside the host mirror
(hc_host_sam_records_to_lines) on the same box and the same seeded records: uniform coverage, 150-base reads, a share with I / D / S,
singles and pairs.  Medians of five after one warm-up each; the spread is max - min of the five.  Writes the figures to --out
(profiles/sam_ingest.md).  Not timed: reading the SAM text (the reader is host code for both sides) and the reference's own
scripts/sam2overlaps.py, which is Python 2 and is not run by this tool."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import haploconduct_amd as hc  # noqa: E402
from haploconduct_amd import _native as N  # noqa: E402
from haploconduct_amd import host  # noqa: E402
from haploconduct_amd.records import SAM_ALN_DTYPE, SAM_CIGAR_PLAIN, SAM_ID_PLAIN, SAM_NONE, SAM_OP_DTYPE, SAM_REC_DTYPE  # noqa: E402

L = 150


def synth(seed, n_single, n_pair, coverage):
    rng = np.random.default_rng(seed)
    n_aln = n_single + 2 * n_pair
    genome = max(1000, int(n_aln * L / coverage))
    kind = rng.choice(4, n_aln, p=[0.7, 0.1, 0.1, 0.1])  # all M; aM bI cM; aM bD cM; sS (L - s)M
    a = rng.integers(10, L - 20, n_aln)
    b = rng.integers(1, 4, n_aln)
    counts = np.zeros((n_aln, 3), np.uint32)
    letters = np.zeros((n_aln, 3), np.uint32)
    n_ops = np.where(kind == 0, 1, np.where(kind == 3, 2, 3))
    M, I, D, S = ord("M"), ord("I"), ord("D"), ord("S")
    counts[kind == 0, 0], letters[kind == 0, 0] = L, M
    k = kind == 1
    counts[k, 0], counts[k, 1], counts[k, 2] = a[k], b[k], L - a[k] - b[k]
    letters[k] = (M, I, M)
    k = kind == 2
    counts[k, 0], counts[k, 1], counts[k, 2] = a[k], b[k], L - a[k]
    letters[k] = (M, D, M)
    k = kind == 3
    counts[k, 0], counts[k, 1] = b[k], L - b[k]
    letters[k, 0], letters[k, 1] = S, M
    keep = np.arange(3)[None, :] < n_ops[:, None]
    ops = np.zeros(int(n_ops.sum()), SAM_OP_DTYPE)
    ops["count"], ops["letter"] = counts[keep], letters[keep]
    alns = np.zeros(n_aln, SAM_ALN_DTYPE)
    alns["len"], alns["op_count"] = L, n_ops
    alns["op_first"] = np.concatenate(([0], np.cumsum(n_ops)[:-1]))
    alns["marks"] = SAM_ID_PLAIN | SAM_CIGAR_PLAIN
    pos = rng.integers(1, genome, n_single + n_pair)
    alns["cpos"][:n_single] = pos[:n_single]
    alns["flag"][:n_single] = rng.choice((0, 16), n_single)
    alns["id"][:n_single] = np.arange(n_single)
    first = n_single + 2 * np.arange(n_pair)
    alns["cpos"][first] = pos[n_single:]
    alns["cpos"][first + 1] = pos[n_single:] + rng.integers(0, 2 * L, n_pair)
    alns["id"][first] = alns["id"][first + 1] = n_single + np.arange(n_pair)
    alns["ref"][first + 1] = SAM_NONE
    recs = np.zeros(n_single + n_pair, SAM_REC_DTYPE)
    recs["first"][:n_single], recs["second"][:n_single] = np.arange(n_single), SAM_NONE
    recs["first"][n_single:], recs["second"][n_single:] = first, first + 1
    recs["reverse"][n_single:] = rng.random(n_pair) < 0.3
    return host.SamRecords(alns, recs, ops, [genome]), genome


def timed(fn, reps):
    fn()  # warm-up: code objects, page-locked blocks, the allocations that only grow
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--coverage", type=float, default=60.0)
    ap.add_argument("--min-overlap-len", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/sam_ingest.md")
    args = ap.parse_args()
    n_single = args.records // 2
    n_pair = args.records - n_single
    sam, genome = synth(7, n_single, n_pair, args.coverage)
    mol = args.min_overlap_len
    piece = 1 << 18  # what the stage hands a text block at a time
    state = {}
    with hc.EdgeScorer(hc.Settings()) as sc:
        t0 = time.perf_counter()
        sc.set_sam_records(sam)
        t_upload = time.perf_counter() - t0

        def device():
            n = sc.sam_plan(mol)
            p = C.c_void_p()
            for at in range(0, n, piece):  # every range, as the stage asks for them; the lines stay in device memory
                N.check(N.lib.hc_sam_lines_slot(sc._ctx, 0, at, min(piece, n - at), C.byref(p)), "hc_sam_lines_slot")
            state["lines"] = n

        def plan_only():
            sc.sam_plan(mol)

        v = sam._view()

        def mirror():
            n = C.c_uint64()
            N.check(N.lib.hc_host_sam_records_to_lines(C.byref(v), mol, None, None, 0, C.byref(n)), "hc_host_sam_records_to_lines")
            state["mirror_lines"] = n.value

        t_dev = timed(device, args.reps)
        t_plan = timed(plan_only, args.reps)
        t_host = timed(mirror, args.reps)
        cand, window = sc.sam_plan_counts()
        assert state["lines"] == state["mirror_lines"], (state["lines"], state["mirror_lines"])
        # the same lines: all of them up to 4 * 10^6, else the first and the last 10^6
        want, _ = sam.to_lines(mol)
        n = state["lines"]
        spans = [(0, n)] if n <= 4000000 else [(0, 1000000), (n - 1000000, 1000000)]
        for at, k in spans:
            assert sc.sam_lines(at, k).tobytes() == want[at:at + k].tobytes(), "device lines differ from the mirror's"
    med, spread = (lambda ts: float(np.median(ts))), (lambda ts: max(ts) - min(ts))
    slower = t_host if med(t_host) > med(t_dev) else t_dev
    gain = abs(med(t_host) - med(t_dev)) > 3 * spread(slower)
    text = ["# SAM ingest: the enumeration on the device beside the host mirror", "",
            f"`python tools/sam_bench.py --records {args.records} --coverage {args.coverage:g} --min-overlap-len {mol}` on one MI355X box (the mirror on that box's CPU, one thread).",
            "", f"Seeded records: {n_single} singles, {n_pair} pairs of {L}-base reads over {genome} reference bases, 30 % with an I, a D or a leading S.",
            f"Evaluated pairs (sum of e_j - j): {cand}.  Records the waves looked at (sum of i - lo_i): {window}.  Lines: {state['lines']}.",
            f"Upload of the records (hc_set_sam_records, once, not in the figures below): {t_upload * 1e3:.1f} ms.", "",
            "| what | median of five (ms) | spread, max - min (ms) | all five (ms) |", "|---|---|---|---|"]
    for name, ts in (("device: plan + all line ranges", t_dev), ("device: plan alone", t_plan), ("host mirror", t_host)):
        text.append(f"| {name} | {med(ts) * 1e3:.2f} | {spread(ts) * 1e3:.2f} | {' '.join(f'{t * 1e3:.2f}' for t in ts)} |")
    text += ["", f"Difference of the medians: {abs(med(t_host) - med(t_dev)) * 1e3:.2f} ms; three times the slower side's spread: {3 * spread(slower) * 1e3:.2f} ms: "
             + (f"a gain of {max(med(t_host), med(t_dev)) / min(med(t_host), med(t_dev)):.1f} x for the {'device' if med(t_dev) < med(t_host) else 'mirror'}." if gain else "no gain is claimed."),
             "The device lines were compared with the mirror's in the same run (equal).",
             "Not measured: reading the SAM text (host code on both sides) and the reference's own `scripts/sam2overlaps.py` (Python 2, not installed where this was measured).", ""]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))


if __name__ == "__main__":
    main()
