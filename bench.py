#!/usr/bin/env python3
"""bench.py — candidate overlaps scored per second in the edge-calculation stage.

    python bench.py --gpus N --steps K --warmup W            (N = 1)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path (hc_score_cands_device: compute_overlap + overlap_score + admission
class for every candidate) over one device-resident batch of synthetic candidates, in the record form the stage
sends to the device (hc_cand_rec, 16 bytes).  Workload = the configuration BASELINE.json's target is quoted on, which
fits one GPU: configs[2] "c3" — 500k synthetic 2x150 bp read pairs, 1e8 p-p candidate overlaps (--max_ov's default,
src/ViralQuasispecies.cpp:58).  N > 1: --scaling strong (default, round 5: the ONE set of 1e8 candidates is split over the ranks
— BASELINE configs[2], what the target's "scaling at 8 GPUs" is quoted on) or weak (every rank scores its own 1e8-candidate set
against the replicated read store; reported under "weak" in the same line); the non-dropped records of every rank are
collected on every rank once per step over RCCL, --gather ring (one all-gather of a fixed-capacity payload) or
direct (all-gather-v: counts, then grouped per-peer send / recv); by default both forms run, each a full leg, the faster is `value`.

Prints ONE JSON line (rank 0) with the contract fields plus
  "roofline":     everything measured in THIS run unless said otherwise: `kernel` (the symbol the library picked,
                  hc_get_kernel_info) and `kernel_ms` (mean launch time, hipEvents on the launch stream);
                  `frac_encoded` = the bytes the kernel must touch in the store's own encoding with no reuse —
                  16 B record + 24 B result + 2 symbols per overlapped position — / kernel_ms / 8 TB/s;
                  `frac_8d` = SURVEY.md 8(d)'s 32 + 16 + 4 B per position (ASCII base + quality of both reads) the
                  same way: NOT A BOUND, it exceeds 1 because the store holds one fused symbol byte per position;
                  `achieved` / `frac` / `traffic` = memory-side bytes per launch from the committed PMC passes
                  (profiles/traffic_<workload>.json: FETCH_SIZE x2 + WRITE_SIZE, Infinity-Cache hits included — fabric
                  traffic, not DRAM traffic) / kernel_ms / 8 TB/s — null unless that file was collected on the kernel
                  sources of this run (hash), names the kernel this run launched, and its duration is within 5 % of
                  this run's; `bound` = the busiest unit by the same file's counters ("valu": the kernel is
                  issue-bound), with the busy fractions under `busy`
  "parity":       what the timed region computed, checked in this run (outside the timed region): the results buffer is
                  filled with a pattern before the timed steps; afterwards its digest (a position-dependent 64-bit sum over
                  every record, computed on the device) must equal the digest of an untimed launch into another buffer, and
                  `parity_checked_records` records (four stretches spread over the batch) are compared bit for bit with the CPU
                  oracle (x1, x2, mm, n, class, score, mismatch rate); `edges` = admitted candidates of the step
  "stage_end_to_end": text overlaps file + FASTQ -> populated, sorted OverlapGraph (hc_ec_construct_edges_sorted):
                  median and best of the runs, open + construct totals
  "cpu_baseline": the reference's own process_overlaps (fragment probe) / the CPU oracle timed on this box's host cores;
                  "stage": the reference's own construct_edges + sortEdges (same probe) MEASURED on a file of the first
                  2 000 000 lines of the workload, thread count swept
  "also":         the same measurements on configs[1] "c2" (2M candidates), the round-1 headline
N > 1 adds "ranks": per rank kernel_ms, step_ms, gather_ms (the exchange alone: events on its side stream), gather_wait_ms, and
`n_ranks_seen` = the world size RCCL reported (the run fails if it is not N); the other scaling mode under its name ("weak": every rank
its own set), so one driver pass yields both curves; "gather_modes": both forms of the exchange.
"summary" (last key): the line's figures once more, compact.

Everything above but the contract fields, "config" and the summary needs --full (off by default): "roofline", "parity", "stage_*",
"cpu_baseline", "also", and at N > 1 the other scaling mode and the per-rank kernel times.  A plain run sets up, warms up, times the
steps, writes --dump-outputs and prints the line; it builds the headline's candidate records on the device (paired_candidates_device).
At N > 1 a plain run still times every form of the exchange it is given (--gather): `value` is the fastest of them.
"""
import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
STREAMED_READ_GBS = 6030.0  # a 4 GiB lane-linear read on this chip (profiles/r02_fetch_calibration.jsonl; the guide: ~6.3 TB/s achievable)
# What the PMC counters count is the L2's memory-side (fabric) traffic, Infinity-Cache hits included; the ceiling for THAT, in this
# kernel's access shape (random rows of a read store of a few hundred MB gathered into LDS), is the guide's measured gather rate,
# MI355X_MICROARCH.md "Indexed rows: gather into LDS": 7.4 - 7.9 TB/s chip-wide for a 151 MB table (8.6 from a 38 MB one, 6.0 - 6.1
# for a 1.2 GB table swept from HBM).  The lower end is used.
FABRIC_GATHER_GBS = 7400.0


KERNEL_SOURCES = ("hc_kernels.hip", "hc_device.h", "hc_resolve.h")


def kernel_source_sha():
    """Hash of the sources the scoring kernel is compiled from: a PMC file collected on other sources is stale."""
    import hashlib

    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        with open(os.path.join(ROOT, "haploconduct_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_profile(workload, order, kernel_symbol, kern_ms):
    """The committed rocprofv3 PMC passes of the scoring kernel on this workload (profiles/traffic_<workload>.json,
    produced by tools/collect_traffic.sh: FETCH_SIZE and WRITE_SIZE in separate --pmc passes; FETCH_SIZE doubled as
    MI355X_MICROARCH.md §HBM prescribes for gfx950) — only if it describes what this run measures: collected on the same
    kernel sources, the same kernel symbol, a duration within 5 % of this run's.  Returns (profile or None, why not)."""
    path = os.path.join(ROOT, "profiles", f"traffic_{workload}.json")
    try:
        with open(path) as f:
            t = json.load(f)
    except Exception:
        return None, f"no profiles/traffic_{workload}.json"
    if t.get("order") != order or t.get("record_bytes", 32) != 16:
        return None, "the PMC file is for another candidate order / record format"
    if t.get("kernel_source_sha") != kernel_source_sha():
        return None, f"stale: the PMC file was collected on kernel sources {t.get('kernel_source_sha')}, this run has {kernel_source_sha()}"
    sym = (t.get("kernel") or "").split("(")[0].replace("void ", "").replace("unsigned char", "uint8_t").replace("unsigned short", "uint16_t").strip()
    if sym != kernel_symbol:
        return None, f"the PMC file measured {sym!r}, this run launched {kernel_symbol!r}"
    # the file's two clocks: rocprofv3's kernel trace (average duration) and hipEvents in the same, profiled run (inflated for launches of
    # a fraction of a millisecond); one of them within 5 % of this run's, or this run's between the two
    # the file's clock: the MEDIAN duration of >= 30 traced launches (round 4; the mean of nine with one outlier needed an acceptance
    # window in round 3), else the older files' average / hipEvents pair
    ref = t.get("kernel_ms_rocprof_median") or t.get("kernel_ms_rocprof_avg")
    # hipEvents around back-to-back launches carry the launch gaps: a few per cent of a 0.2 ms kernel; boxes of this pool differ by up to
    # 7 % on the same library (round 6: 6.44 - 6.95 ms at C3): symbol and source hash identify the kernel, the duration guards against a
    # file from another launch size
    tol = 0.08 if kern_ms >= 1.0 else 0.10
    lo = t.get("kernel_ms_rocprof_min")
    # launches of a fraction of a millisecond are stretched by the tracer (C2: minimum 0.141, median 0.171 ms of 63 traced launches for a kernel
    # hipEvents put at 0.145 - 0.153): such a run matches when it lies between the traced minimum and median (5 % either side)
    if ref and lo and kern_ms < 1.0 and 0.95 * lo <= kern_ms <= 1.05 * ref:
        return t, None
    if not ref or abs(ref - kern_ms) > tol * kern_ms:
        return None, f"the PMC file's kernel took {ref} ms (rocprofv3 kernel trace), this run's {kern_ms:.4f} ms: more than {tol:.0%} apart"
    return t, None


def roofline_record(workload, order, n, positions, kern_ms, kernel_info, symbytes):
    """See the module docstring.  `frac` = `achieved` / `peak` with peak = the 8 TB/s HBM spec (the quantity of rounds 1 - 3; round 4 had
    divided by the guide's 7.4 TB/s gather ceiling — that ratio is now `frac_of_fabric_gather`); the numerator is the L2's memory-side
    traffic per launch as the PMC passes count it (Infinity-Cache hits included).  `bound` = the busiest unit by the same file's counters
    ("valu": issue-bound; "hbm": the memory side — the L2's fabric traffic, Infinity-Cache hits included, as a share of the HBM peak).  The algorithmic figures (`frac_encoded`, `frac_8d`)
    need no counters."""
    kernel_symbol = kernel_info.split(" encoding=")[0]
    t_s = kern_ms * 1e-3
    bytes_8d = 48 * n + 4 * positions                   # 32 B record + 16 B result + 4 B per overlapped position
    bytes_enc = (16 + 24) * n + 2 * symbytes * positions  # hc_cand_rec + hc_result_rec + one symbol of each read per position
    r = {"bound": "unmeasured (no matching PMC file)", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
         "peak_is": "the HBM spec peak (MI355X_MICROARCH.md: 8 TB/s)", "fabric_gather_peak": FABRIC_GATHER_GBS,
         "fabric_gather_peak_is": "the measured chip-wide rate of random-row gathers into LDS from a table of this size class (MI355X_MICROARCH.md, "
                                  "'Indexed rows: gather into LDS': 7.4 - 7.9 TB/s at 151 MB; lower end) — the ceiling for what `traffic` counts",
         "kernel": kernel_symbol, "kernel_info": kernel_info, "kernel_ms": kern_ms, "kernel_candidates_per_s": n / t_s,
         "kernel_positions_per_s": positions / t_s, "kernel_source_sha": kernel_source_sha(),
         "encoded_bytes_per_launch": bytes_enc, "encoded_GBps": bytes_enc / t_s / 1e9, "frac_encoded": bytes_enc / t_s / 1e9 / HBM_PEAK_GBS,
         "bytes_8d_per_launch": bytes_8d, "GBps_8d": bytes_8d / t_s / 1e9, "frac_8d": bytes_8d / t_s / 1e9 / HBM_PEAK_GBS,
         "frac_8d_note": "not a bound: SURVEY 8(d) counts an ASCII base and a quality byte per read and position; the store holds one fused symbol "
                         "and neighbouring candidates share reads (L1/L2), so the figure exceeds 1 of the HBM peak",
         "note": "achieved/traffic: memory-side (fabric) bytes of the PMC passes per launch, FETCH_SIZE x2 + WRITE_SIZE, Infinity-Cache hits "
                 "included (factor checked on known byte counts: profiles/r02_fetch_calibration.jsonl) / kernel_ms of THIS run — only when the PMC "
                 "file matches this run's kernel sources, kernel symbol and duration; frac = achieved / peak (the 8 TB/s HBM spec); "
                 "frac_of_fabric_gather = achieved / 7.4 TB/s; bound = the busiest unit; frac_encoded: compulsory bytes in the store's encoding without cache-reuse credit / "
                 "8 TB/s; busiest_unit: by the same file's counters"}
    t, why = pmc_profile(workload, order, kernel_symbol, kern_ms)
    if not t:
        r["traffic_note"] = why
        return r
    c = t.get("counters_per_launch", {})
    r["traffic"] = t["hbm_bytes_per_launch"]
    r["achieved"] = t["hbm_bytes_per_launch"] / t_s / 1e9
    r["frac"] = r["achieved"] / HBM_PEAK_GBS
    r["bound"] = "hbm"  # replaced below by the busiest unit when the file has the counters
    r["frac_of_hbm_peak"] = r["frac"]
    r["frac_of_fabric_gather"] = r["achieved"] / FABRIC_GATHER_GBS
    r["frac_of_streamed_read"] = r["achieved"] / STREAMED_READ_GBS
    r["traffic_source"] = {"file": f"profiles/traffic_{workload}.json", "git_sha": t.get("git_sha"), "kernel_source_sha": t.get("kernel_source_sha"),
                           "kernel_ms_rocprof_median": t.get("kernel_ms_rocprof_median"), "kernel_ms_rocprof_avg": t.get("kernel_ms_rocprof_avg"),
                           "kernel_launches_traced": t.get("kernel_launches_traced"),
                           "kernel_ms_hipevents_under_rocprof": t.get("kernel_ms_hipevents_under_rocprof")}
    busy = {}
    if c.get("GRBM_GUI_ACTIVE"):
        cycles = c["GRBM_GUI_ACTIVE"] / 8.0  # the counter sums the 8 XCDs
        n_cu = 256
        busy["hbm"] = r["frac"]  # the memory side: fabric bytes (Infinity-Cache hits included) against the HBM peak
        if c.get("TA_BUSY_avr"):
            busy["ta"] = c["TA_BUSY_avr"] / cycles  # vector-memory front end (address processing of the gathers)
        if c.get("SQ_ACTIVE_INST_VALU"):
            busy["valu"] = c["SQ_ACTIVE_INST_VALU"] * 4.0 / (4 * n_cu * cycles)  # quad-cycles over all SIMDs
        if c.get("SQ_LDS_IDX_ACTIVE"):
            busy["lds"] = c["SQ_LDS_IDX_ACTIVE"] / (n_cu * cycles)
        r["busiest_unit"] = max(busy, key=busy.get)
        r["bound"] = r["busiest_unit"]
        busy["kernel_cycles"] = cycles
        if c.get("SQ_WAVE_CYCLES"):
            busy["waves_resident_per_cu"] = c["SQ_WAVE_CYCLES"] * 4.0 / (n_cu * cycles)  # quad-cycles of resident waves over the CUs' cycles (16 = full)
        if c.get("SQ_LDS_BANK_CONFLICT") is not None and c.get("SQ_LDS_IDX_ACTIVE"):
            busy["lds_bank_conflict_share"] = c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"]
    if c.get("TCC_HIT_sum") is not None and c.get("TCC_MISS_sum"):
        busy["l2_hit_rate"] = c["TCC_HIT_sum"] / (c["TCC_HIT_sum"] + c["TCC_MISS_sum"])
    if c.get("SQ_INSTS_VALU") and c.get("SQ_INSTS_VMEM_RD"):
        per_wave = c["SQ_INSTS_VALU"] / (n / 64.0)  # what every lane, i.e. every candidate, executes
        busy["valu_instructions_per_candidate"] = per_wave
        busy["valu_instructions_per_position"] = per_wave / (positions / max(n, 1))
        busy["vmem_read_instructions_per_wave"] = c["SQ_INSTS_VMEM_RD"] / (n / 64.0)
    r["busy"] = busy
    return r


_WORKLOADS = {}
_CAND_MEMO = {}
PAIRED_WORKLOAD = re.compile(r"^(c2|c2-small|c2-mid|c2-100k|c3|c3-lite)(q(\d+)(r?))?$")


def cached_candidates(key, make):
    """HC_WORKLOAD_CACHE=<dir>: the candidate records of a synthetic workload are kept there between processes (the PMC passes of
    tools/collect_traffic.sh run one process per counter group over the same 10^8 candidates: a minute of numpy each time).  The key names
    everything the records depend on; unset: generated every time."""
    if _CAND_MEMO.get("key") == key:  # the q<K> variants of a configuration score the configuration's own candidates
        return _CAND_MEMO["cand"]
    d = os.environ.get("HC_WORKLOAD_CACHE")
    if not d:
        cand = make()
        _CAND_MEMO.update(key=key, cand=cand)
        return cand
    path = os.path.join(d, "cand_" + "_".join(str(k) for k in key) + ".npy")
    if os.path.exists(path):
        cand = np.load(path)
        _CAND_MEMO.update(key=key, cand=cand)
        return cand
    cand = make()
    _CAND_MEMO.update(key=key, cand=cand)
    os.makedirs(d, exist_ok=True)
    tmp = path + f".{os.getpid()}.tmp.npy"
    np.save(tmp, cand)
    os.replace(tmp, path)
    return cand


def paired_candidates_device(meta, n_candidates, seed, min_len=75, max_window=100000):
    """synth.paired_candidates(meta, n_candidates, min_len, seed, max_window) of untrimmed pairs as the hc_cand_rec records
    EdgeScorer.pack_cands makes of it, bit for bit, in an int32 [n, 4] device tensor.  The window walk and the seeded draw are the host's;
    the sorts, gathers and packing run on the device: on the host, the stable argsort of 10^8 keys and the record assembly took most of a
    minute.  Every pair of reads is met once, at one distance in start order, so the sfo keys are unique and any sort orders them as the
    host's does.  tests/test_gpu_bench_records.py and tests/test_gpu_c3.py keep it equal to the host's records."""
    import torch

    s, e, flipped, rl = meta["s"], meta["e"], meta["flipped"], meta["read_len"]
    order = np.argsort(s, kind="stable").astype(np.int32)
    ss, ee = s[order].astype(np.int32), e[order].astype(np.int32)
    maxd = rl - min_len
    out_i, out_j, out_p1, out_d2 = [], [], [], []
    for k in range(1, min(ss.size, max_window)):
        ds = ss[k:] - ss[:-k]
        m = ds <= maxd
        if not m.any():
            break
        d2 = ee[k:] - ee[:-k]
        m &= np.abs(d2) <= maxd
        idx = np.nonzero(m)[0]
        out_i.append(order[idx])
        out_j.append(order[idx + k])
        out_p1.append(ds[idx].astype(np.int16))
        out_d2.append(d2[idx].astype(np.int16))
    dev = torch.device("cuda")
    i, j, p1, d2 = (torch.from_numpy(np.concatenate(x)).to(dev).int() for x in (out_i, out_j, out_p1, out_d2))
    del out_i, out_j, out_p1, out_d2
    if i.numel() < n_candidates:
        raise ValueError(f"only {i.numel()} candidates exist, {n_candidates} requested: lower genome_len")
    if i.numel() > n_candidates:
        pick = np.random.default_rng(seed).choice(i.numel(), n_candidates, replace=False)
        keep = torch.zeros(i.numel(), dtype=torch.bool, device=dev)
        keep[torch.from_numpy(pick).to(dev)] = True
        del pick
        i, j, p1, d2 = i[keep], j[keep], p1[keep], d2[keep]  # in index order, as the host's sorted pick
        del keep
    o = torch.argsort((torch.minimum(i, j).long() << 32) | torch.maximum(i, j).long(), stable=True)
    i, j, p1, d2 = i[o], j[o], p1[o], d2[o]
    del o
    fl = torch.from_numpy(flipped).to(dev)
    # hc_pack_cands: pos1 | ori1 << 28 | ori2 << 29 | ord code << 30 ('1' -> 1, '2' -> 2); |pos| <= read_len - min_len needs no clamp
    bits = p1 | torch.where(fl[i.long()], 0, 1 << 28) | torch.where(fl[j.long()], 0, 1 << 29) | torch.where(d2 >= 0, 1 << 30, -(1 << 31))
    return torch.stack([i, j, bits.int(), d2.abs()], dim=1)


def build_workload(workload, rank, keep=False, on_device=False):
    """BASELINE.json configs; candidates in sfo2overlaps order.  keep: remember the (one) latest workload built, so that
    a second leg over the same candidates does not generate them again.  on_device: the candidates as the hc_cand_rec records a step
    reads, in an int32 [n, 4] device tensor, instead of host hc_overlap_rec records."""
    if keep:
        if (workload, rank, on_device) not in _WORKLOADS:
            _WORKLOADS.clear()
            _WORKLOADS[(workload, rank, on_device)] = build_workload(workload, rank, on_device=on_device)
        return _WORKLOADS[(workload, rank, on_device)]
    from haploconduct_amd import synth
    import haploconduct_amd as hc

    st = dict(edge_threshold=0.97, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=150)
    pw = PAIRED_WORKLOAD.match(workload)
    if pw:
        # <base>[q<K>[r]]: the base configuration's pairs and candidates with K distinct quality values — uniform i.i.d. (the HC_C4_K idea at
        # the north-star size: K = 25 -> the LG = 5 table, 35 -> the wide 8-bit table, 60 -> 16-bit symbols), or with `r` drawn from the
        # histogram of the reference's example reads that has K values (tests/golden/quality_histograms.json: 35 = polyte/example
        # forward.fastq, 25 = savage/example singles.fastq, 20 = its paired1.fastq).  Bases, fragments and candidates are the base
        # configuration's own (synth.make_paired_dataset draws the qualities last).
        base, nq, real = pw.group(1), pw.group(3), bool(pw.group(4))
        n_pairs, glen, n_cand = {"c2": (50000, 45000, 2000000), "c2-small": (5000, 1800, 200000), "c2-mid": (50000, 45000, 400000), "c2-100k": (50000, 45000, 100000),
                                 "c3": (500000, 90000, 100000000), "c3-lite": (500000, 90000, 20000000)}[base]
        quals, qual_p, qdesc = None, None, "6 quality values (SURVEY 8(d))"
        if nq:
            nq = int(nq)
            if real:
                with open(os.path.join(ROOT, "tests", "golden", "quality_histograms.json")) as f:
                    hists = json.load(f)
                pick = [h for h in hists.values() if h["distinct"] == nq]
                if not pick:
                    raise SystemExit(f"no example-read histogram with {nq} quality values (have {sorted(h['distinct'] for h in hists.values())})")
                quals = np.array([int(b) for b in pick[0]["counts"]], dtype=np.uint8)
                qual_p = np.array(list(pick[0]["counts"].values()), dtype=np.float64)
                qdesc = f"{nq} quality values drawn from the histogram of the reference's {pick[0]['source']}"
            else:
                if not 1 <= nq <= 93:
                    raise SystemExit("q<K>: 1 <= K <= 93")
                quals = (np.arange(1, nq + 1) + 33).astype(np.uint8)
                qdesc = f"{nq} quality values, uniform i.i.d."
        reads, meta = synth.make_paired_dataset(n_pairs, glen, seed=1, quals=quals, qual_p=qual_p)
        if on_device:
            cand = paired_candidates_device(meta, n_cand, seed=2 + rank)
        else:
            cand = cached_candidates(("paired", n_pairs, glen, n_cand, 2 + rank), lambda: synth.paired_candidates(meta, n_candidates=n_cand, seed=2 + rank))
        desc = f"{workload}: {n_pairs} synthetic 2x150 bp read pairs, {qdesc}, {n_cand} p-p candidates per GPU"
        cfg = {"read_pairs": n_pairs, "genome_len": glen, "quality_alphabet": int(np.count_nonzero(np.bincount(reads.quals, minlength=256)))}
    elif workload == "c4":
        # POLYTE diploid 20x per haplotype, 2x250 bp, every read a single (polyte.py:283-288), both orientations,
        # edge_threshold 1 / merge_contigs 0 (polyte.py:617-626), 35 distinct quality values as in polyte/example
        glen, cov = 400000, 40
        n_reads = glen * cov // 250
        nq = int(os.environ.get("HC_C4_K", "35"))  # distinct quality values (35 as in polyte/example)
        quals = (np.arange(1, nq + 1) + 33).astype(np.uint8)
        reads, meta = synth.make_single_dataset(n_reads, glen, len_lo=250, len_hi=250, n_strains=2, divergence=0.001,
                                                flip_frac=0.5, seed=4, quals=quals)
        cand = synth.single_candidates(meta, min_overlap=127)
        st = dict(edge_threshold=1.0, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=127)
        desc = f"c4: {n_reads} synthetic 250 bp reads as singles (diploid, 20x per haplotype), {cand.size} s-s candidates"
        cfg = {"reads": n_reads, "genome_len": glen, "quality_alphabet": nq}
    elif workload == "c5":
        # mixed-length contig + read re-overlap (SAVAGE stage b/c): log-uniform 150..6000 bp singles
        n_reads, glen = 60000, 300000
        reads, meta = synth.make_single_dataset(n_reads, glen, len_lo=150, len_hi=6000, n_strains=3, divergence=0.01,
                                                flip_frac=0.5, seed=5, log_uniform=True)
        cand = synth.single_candidates(meta, min_overlap=100, n_candidates=2000000)
        st = dict(edge_threshold=0.995, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=100)
        desc = f"c5: {n_reads} synthetic singles of log-uniform length 150..6000 bp, {cand.size} s-s candidates"
        cfg = {"reads": n_reads, "genome_len": glen}
    elif workload == "c6":
        # tuning workload: contig-length sequences of ONE length (no bucketing): which occupancy / fetch form long rows want
        n_reads, glen = 40000, 300000
        reads, meta = synth.make_single_dataset(n_reads, glen, len_lo=2000, len_hi=2000, n_strains=3, divergence=0.01, flip_frac=0.5, seed=7)
        cand = synth.single_candidates(meta, min_overlap=100, n_candidates=1500000)
        st = dict(edge_threshold=0.995, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=100)
        desc = f"c6: {n_reads} synthetic singles of 2000 bp, {cand.size} s-s candidates"
        cfg = {"reads": n_reads, "genome_len": glen}
    elif workload == "c2t":
        # tuning workload: quality-trimmed pairs — mates of 60..150 bp (mixed sequence lengths in a PAIRED set), p-p candidates
        reads, meta = synth.make_paired_dataset(50000, 45000, seed=1, trim_lo=60)
        cand = synth.paired_candidates(meta, n_candidates=None, min_len=50, seed=2)
        cand = cand[:2000000]
        st = dict(edge_threshold=0.97, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=100)
        desc = f"c2t: 50000 synthetic pairs trimmed to 60..150 bp per mate, {cand.size} p-p candidates"
        cfg = {"read_pairs": 50000, "genome_len": 45000}
    elif workload == "c1s":
        # the SAVAGE-example shape at timing size: merged single-end reads of 400..500 bp (savage/example/input_fas/singles.fastq: 2 000
        # of them beside 200 pairs), s-s candidates, stage-a settings (savage.py:384: --edge_threshold 0.97, M = 200)
        n_reads, glen = 100000, 300000
        reads, meta = synth.make_single_dataset(n_reads, glen, len_lo=400, len_hi=500, n_strains=3, divergence=0.01, flip_frac=0.5, seed=8)
        cand = synth.single_candidates(meta, min_overlap=200, n_candidates=2000000)
        st = dict(edge_threshold=0.97, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=200)
        desc = f"c1s: {n_reads} synthetic singles of 400..500 bp (the SAVAGE example's merged reads), {cand.size} s-s candidates"
        cfg = {"reads": n_reads, "genome_len": glen}
    elif workload in ("c5s", "c5m", "c5t"):
        # tuning workloads for the dispatch between the plain and the length-bucketed launch: reads of mixed but short / medium length
        lo, hi = {"c5s": (100, 400), "c5m": (150, 1500), "c5t": (120, 900)}[workload]
        n_reads, glen = 120000, 300000
        reads, meta = synth.make_single_dataset(n_reads, glen, len_lo=lo, len_hi=hi, n_strains=3, divergence=0.01, flip_frac=0.5, seed=6, log_uniform=True)
        cand = synth.single_candidates(meta, min_overlap=60, n_candidates=2000000)
        st = dict(edge_threshold=0.995, ov_threshold=0.9, merge_contigs=0.0, min_overlap_len=60)
        desc = f"{workload}: {n_reads} synthetic singles of log-uniform length {lo}..{hi} bp, {cand.size} s-s candidates"
        cfg = {"reads": n_reads, "genome_len": glen}
    else:
        raise SystemExit(f"unknown workload {workload}")
    if on_device and not pw:
        import torch

        cand = torch.from_numpy(hc.EdgeScorer.pack_cands(cand).view(np.int32).reshape(-1, 4)).cuda()
    cfg = dict(cfg, workload=desc, candidates_per_gpu=len(cand))
    return reads, cand, cfg, hc.Settings(**st)


def cpu_baseline(reads, settings, cand, budget_s=12.0):
    """The oracle (a port of the reference algorithm) on the host cores, ~budget_s of CPU wall time.
    The thread count is the fastest of {all, 1/2, 1/4, 1/8 of the hardware threads} on a short probe
    (like the reference, the port allocates per overlap and stops scaling when the allocator saturates)."""
    from tests import _oracle

    hw = os.cpu_count() or 1
    sample = cand[: min(cand.size, 1000000)]
    probe = sample[: min(sample.size, 200000)]
    best_t, best_rate = hw, 0.0
    for t in sorted({max(1, hw // d) for d in (1, 2, 4, 8)}, reverse=True):
        _oracle.score_batch(reads, settings, probe[:20000], n_threads=t)  # spin the OpenMP team up
        t0 = time.perf_counter()
        _oracle.score_batch(reads, settings, probe, n_threads=t)
        rate = probe.size / (time.perf_counter() - t0)
        if rate > best_rate:
            best_t, best_rate = t, rate
    done, t0 = 0, time.perf_counter()
    while True:
        _oracle.score_batch(reads, settings, sample, n_threads=best_t)
        done += sample.size
        dt = time.perf_counter() - t0
        if dt >= budget_s:
            break
    return {"value": done / dt, "unit": "candidate overlaps/s", "cores": best_t, "kind": "port",
            "sample": f"{done} candidates ({done // sample.size} passes over the first {sample.size} of the rank-0 batch), "
                      f"oracle/hc_oracle.c with {best_t} OpenMP threads (fastest of 1, 1/2, 1/4, 1/8 of {hw} hardware threads), "
                      f"{dt:.1f} s"}


_REF_PROBE = {}


def _ref_probe(reads):
    """oracle/_ref/libhcref_edgecalc_omp.so (the reference's own lines compiled verbatim behind declaration-only class shells, g++ -O2
    -fopenmp; built in the build container, it travels with the repository) and the read set in the form its entry points take.
    None when the library is not there."""
    import ctypes as C

    lib_path = os.path.join(ROOT, "oracle", "_ref", "libhcref_edgecalc_omp.so")
    if not os.path.exists(lib_path):
        return None
    key = id(reads)
    if key not in _REF_PROBE:
        ref = C.CDLL(lib_path)
        seqs, quals = zip(*(reads.seq(q) for q in range(reads.n_seq)))
        S, Q = (C.c_char_p * len(seqs))(*seqs), (C.c_char_p * len(quals))(*quals)
        ids = np.ascontiguousarray(reads.read_ids, dtype=np.uint64)
        n_single = sum(1 for r in range(reads.n_reads) if not reads.is_paired(r))
        _REF_PROBE.clear()
        _REF_PROBE[key] = (ref, S, Q, ids, n_single, (seqs, quals))
    return _REF_PROBE[key][:5]


class _FragSettings(ctypes.Structure):  # frag_ec_settings of oracle/ref_ec_postlude.inc
    _fields_ = [("edge_threshold", ctypes.c_double), ("ov_threshold", ctypes.c_double), ("merge_contigs", ctypes.c_double),
                ("mismatch", ctypes.c_double), ("min_read_len", ctypes.c_uint32), ("ignore_inclusions", ctypes.c_uint32)]


def cpu_baseline_reference(reads, settings, cand, budget_s=10.0, n_lines=200000):
    """The REFERENCE'S OWN process_overlaps — compute_overlap, overlap_score, the OpenMP loop, the serial insert, the
    nonedge file (src/EdgeCalculator.cpp:26-557 and the OverlapGraph methods it calls) — timed on the host cores.
    Returns None when the probe library is not there."""
    import ctypes as C
    import tempfile

    from haploconduct_amd import synth

    probe = _ref_probe(reads)
    if not probe:
        return None
    ref, S, Q, ids, n_single = probe
    vp = C.c_void_p
    ref.frag_time_process_overlaps.restype = C.c_int
    ref.frag_time_process_overlaps.argtypes = [C.POINTER(_FragSettings), vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.c_char_p, C.c_int,
                                               C.c_int, vp, C.POINTER(C.c_uint64)]
    sample = cand[: min(cand.size, n_lines)]
    lines = synth.records_to_lines(sample, reads)
    fields = [f.encode() for ln in lines for f in ln.split("\t")]
    L = (C.c_char_p * len(fields))(*fields)
    fs = _FragSettings(settings.edge_threshold, settings.ov_threshold, settings.merge_contigs, settings.mismatch, settings.min_read_len, 0)
    hw = os.cpu_count() or 1
    edges = C.c_uint64()

    def run(threads, reps):
        secs = np.zeros(reps, np.float64)
        with tempfile.TemporaryDirectory() as d:
            rc = ref.frag_time_process_overlaps(C.byref(fs), S, Q, ids.ctypes.data, n_single, reads.n_reads - n_single, L, len(lines), d.encode(),
                                                threads, reps, secs.ctypes.data, C.byref(edges))
        assert rc == 0
        return secs

    # fixed thread counts on the full sample (round 5: the round-4 sweep picked a count on one short run and the figure wandered 1.1 - 1.9e6
    # with the pick): every count gets the same share of the budget, the best is `value`, all of them are reported
    # round 6: the smallest count (32 threads, the fastest on every box so far) runs for the whole budget_s (>= 10 s: the driver's and the
    # builder's runs of round 5 differed by 19 % on 3 s), the others for a quarter of it each
    counts = sorted({t for t in (32, 64, 128) if t <= hw} or {hw})
    per_threads = {}
    for t in counts:
        first = float(run(t, 1)[0])  # spins the OpenMP team up and sizes the repetitions
        share = budget_s if t == counts[0] else budget_s / 4.0
        reps = int(max(2, min(200, share / max(first, 1e-3))))
        secs = run(t, reps)
        per_threads[t] = {"value": len(lines) * reps / float(secs.sum()), "reps": reps, "seconds": float(secs.sum()),
                          "best_rep_value": len(lines) / float(secs.min())}
    best_t = max(per_threads, key=lambda t: per_threads[t]["value"])
    b = per_threads[best_t]
    return {"value": b["value"], "unit": "candidate overlaps/s", "cores": best_t, "kind": "reference",
            "by_threads": {str(t): v for t, v in per_threads.items()},
            "sample": f"{b['reps']} x {len(lines)} candidates (the first of the rank-0 batch) through the reference's own process_overlaps "
                      f"(src/EdgeCalculator.cpp:26-557 + the OverlapGraph methods it calls: compute_overlap, overlap_score, OpenMP loop, serial "
                      f"insert of {int(edges.value)} edges, nonedge file), compiled verbatim as a fragment probe "
                      f"(oracle/_ref/libhcref_edgecalc_omp.so, g++ -O2 -fopenmp, declaration-only class shells; construct_edges' text parsing "
                      f"is not part of it: see `stage`), at fixed {counts} OpenMP threads of {hw} hardware threads, the best ({best_t}) is `value`, "
                      f"{b['seconds']:.1f} s"}


def cpu_baseline_stage_reference(reads, settings, cand, n_lines=2000000, sweep_lines=250000):
    """The reference's own STAGE, measured: construct_edges (src/EdgeCalculator.cpp:561-666 — getline, the tab tokeniser, 13 strings and
    an Overlap per line, the prefilter, process_overlaps every 1e6 accepted lines, the rejects' file) followed by sortEdges
    (src/OverlapGraph.cpp:722-764, main calls it right behind: ViralQuasispecies.cpp:297), on an overlaps FILE of the first n_lines
    candidates of the workload, on this box's host cores.  The same fragment probe as above; its two Boost statements (:584 the line
    trim -> a build-owned statement, :587 the --allow_spaced_overlaps split -> never reached) are the only lines that are not the
    reference's.  The FASTQ load is outside the timed calls, as in the reference's own stage timer (ViralQuasispecies.cpp:280-283).
    Thread count: swept on the first sweep_lines lines of the file (--max_ov stops the reference there), then the whole file once
    at the fastest.  Returns None when the probe library is not there."""
    import ctypes as C
    import shutil
    import tempfile

    from haploconduct_amd import host

    probe = _ref_probe(reads)
    if not probe:
        return None
    ref, S, Q, ids, n_single = probe
    vp = C.c_void_p
    ref.frag_time_construct_edges.restype = C.c_int
    ref.frag_time_construct_edges.argtypes = [C.POINTER(_FragSettings), vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p,
                                              C.c_int, C.c_int, vp, vp, C.POINTER(C.c_uint64), vp]
    sample = cand[: min(cand.size, n_lines)]
    fs = _FragSettings(settings.edge_threshold, settings.ov_threshold, settings.merge_contigs, settings.mismatch, settings.min_read_len, 0)
    pre = (C.c_uint32 * 3)(settings.min_overlap_len, settings.min_overlap_perc, 0)
    hw = os.cpu_count() or 1
    d = tempfile.mkdtemp(prefix="hcrefstage_")
    try:
        path = os.path.join(d, "overlaps.txt")
        host.write_overlaps(path, sample, reads)
        text_bytes = os.path.getsize(path)
        edges = C.c_uint64()
        counters = (C.c_uint32 * 3)()

        def run(threads, max_ov):
            cs, ss = np.zeros(1, np.float64), np.zeros(1, np.float64)
            rc = ref.frag_time_construct_edges(C.byref(fs), pre, max_ov, S, Q, ids.ctypes.data, n_single, reads.n_reads - n_single, path.encode(),
                                               d.encode(), threads, 1, cs.ctypes.data, ss.ctypes.data, C.byref(edges), counters)
            assert rc == 0
            return float(cs[0]), float(ss[0])

        sweep = {}
        n_sweep = min(sweep_lines, sample.size)
        for t in sorted({max(1, hw // k) for k in (1, 2, 4, 8, 16, 32)} | {1}, reverse=True):
            c_s, s_s = run(t, n_sweep)
            sweep[t] = n_sweep / (c_s + s_s)
        best_t = max(sweep, key=sweep.get)
        c_s, s_s = run(best_t, 10 ** 9)
        n_edges = int(edges.value)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {"value": sample.size / (c_s + s_s), "unit": "candidate overlaps/s", "cores": best_t, "kind": "reference", "measured": True,
            "lines": int(sample.size), "text_bytes": text_bytes, "construct_edges_s": c_s, "sort_edges_s": s_s, "edges": n_edges,
            "self_overlaps": int(counters[2]), "us_per_line": (c_s + s_s) / sample.size * 1e6,
            "thread_sweep_lines_per_s": {str(k): v for k, v in sorted(sweep.items())},
            "sample": f"the reference's own construct_edges + sortEdges (src/EdgeCalculator.cpp:561-666 minus its two Boost statements, "
                      f"src/OverlapGraph.cpp:722-764; fragment probe oracle/_ref/libhcref_edgecalc_omp.so, g++ -O2 -fopenmp) on a file of the first "
                      f"{sample.size} lines of the workload ({text_bytes} bytes; every line passes the prefilter), once, {best_t} OpenMP threads "
                      f"(fastest of {sorted(sweep)} on the first {n_sweep} lines), {c_s + s_s:.1f} s; compare stage_end_to_end.value"}


def device_digest(torch, d_results, n, chunk=1 << 24):
    """A position-dependent 64-bit digest of n hc_result_rec records (24 bytes: x1 bits, x2 bits, mm | n_cls << 32) on the device:
    sum over i of mix(i) * (x1 ^ rot(x2) ^ rot(w)) in wrapping int64 arithmetic, by pieces of `chunk` records."""
    v = d_results.view(torch.int64).view(-1, 3)
    total = torch.zeros((), dtype=torch.int64, device=d_results.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        w = v[lo:hi]
        i = torch.arange(lo, hi, dtype=torch.int64, device=d_results.device)
        m = (i * -7046029254386353131 + 1442695040888963407) | 1  # odd multiplier per position (wrapping)
        total += (m * (w[:, 0] ^ (w[:, 1] * 31) ^ (w[:, 2] * 1000003))).sum()
    return int(total.item()) & 0xFFFFFFFFFFFFFFFF


DUMP_SAMPLE = 1 << 20  # records --dump-outputs keeps of a larger step: six float64 arrays of 8 MiB, 48 MiB in all


def dump_outputs(torch, d_results, n, out_dir, sample=DUMP_SAMPLE, seed=0x5EED):
    """--dump-outputs: the n hc_result_rec records the last timed step left in d_results — what a caller of hc_score_cands_device receives —
    as float64 .npy files under out_dir: x1, x2, mm, n and cls (the class as the device wrote it), one entry per record.  Up to `sample`
    records: all of them; more: a fixed, seeded sample of `sample` record positions in ascending order, saved as index.npy.  The workloads
    are seeded too, so two builds given the same arguments can be compared file for file."""
    if n > sample:
        idx = np.sort(np.random.default_rng(seed).choice(n, size=sample, replace=False))
    else:
        idx = np.arange(n, dtype=np.int64)
    w = d_results.view(torch.int64).view(-1, 3)[torch.from_numpy(idx).to(d_results.device)].cpu().numpy()
    word = w[:, 2].view(np.uint64)  # mm | n_cls << 32
    n_cls = word >> np.uint64(32)
    arrays = {"index": idx, "x1": w[:, 0].view(np.float64), "x2": w[:, 1].view(np.float64), "mm": word & np.uint64(0xFFFFFFFF),
              "n": n_cls & np.uint64(0x0FFFFFFF), "cls": n_cls >> np.uint64(28)}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def parity_record(torch, sc, reads, settings, cand, d_out, n, digest_timed, digest_untimed, stretches=4, stretch=1 << 18):
    """What the last timed step left in d_out against (a) the digest of an untimed launch into another buffer and (b) the CPU oracle on
    `stretches` stretches of `stretch` records spread over the batch, bit for bit; and the step's admitted-edge count.  Raises on any
    difference: a bench line is printed only for results that are the reference's."""
    from haploconduct_amd.records import RESULT_DTYPE, result_cls, result_n
    from tests import _oracle

    if os.environ.get("HC_BENCH_ABLATION"):  # experiment builds whose results are garbage by construction (tools/experiments/ablate.sh): timing only
        return {"parity": "NOT CHECKED: HC_BENCH_ABLATION is set — this line times an ablation build and is not a measurement of the product",
                "invalid": True, "parity_checked_records": 0, "edges": None}
    if digest_timed != digest_untimed:
        raise SystemExit(f"bench.py: the timed steps left other results than an untimed launch (digest {digest_timed:#x} vs {digest_untimed:#x})")
    stretch = min(stretch, n)
    starts = sorted({int(k * (n - stretch) / max(stretches - 1, 1)) for k in range(stretches)})
    checked = 0
    threads = min(64, os.cpu_count() or 1)
    for lo in starts:
        res = d_out[lo * 24:(lo + stretch) * 24].cpu().numpy().view(RESULT_DTYPE)
        score, mrate, cls = sc.finalize(res)
        ref = _oracle.score_batch(reads, settings, cand[lo:lo + stretch], n_threads=threads)
        ok = ((ref["status"] == 0).all() and np.array_equal(ref["x1"].view(np.uint64), res["x1"].view(np.uint64))
              and np.array_equal(ref["x2"].view(np.uint64), res["x2"].view(np.uint64)) and np.array_equal(ref["n"], result_n(res))
              and np.array_equal(ref["mm"], res["mm"]) and np.array_equal(ref["cls"], cls)
              and np.array_equal(ref["score"].view(np.uint64), score.view(np.uint64))
              and np.array_equal(ref["mismatch_rate"].view(np.uint64), mrate.view(np.uint64)))
        if not ok:
            raise SystemExit(f"bench.py: records [{lo}, {lo + stretch}) of the timed step differ from the CPU oracle")
        checked += stretch
    # admitted candidates of the step: classes EDGE / EDGE_MC as the device set them, the ambiguous band decided by the host's exp()
    w = d_out.view(torch.int64).view(-1, 3)[:n, 2]
    dev_cls = (w >> 60) & 0xF
    sure = int(((dev_cls == 2) | (dev_cls == 3)).sum().item())
    amb = torch.nonzero(dev_cls == 4).squeeze(1)
    n_amb = int(amb.numel())
    edges = sure
    if n_amb:
        res = d_out.view(torch.uint8).view(-1, 24)[amb].cpu().numpy().reshape(-1).view(RESULT_DTYPE)
        _, _, cls = sc.finalize(res)
        edges += int(((cls == 2) | (cls == 3)).sum())
    return {"parity_checked_records": checked, "parity": "bit-exact vs oracle/hc_oracle.c (x1, x2, mm, n, class, score, mismatch rate)",
            "stretches": [[lo, lo + stretch] for lo in starts], "digest": f"{digest_timed:#018x}", "digest_matches_untimed_launch": True,
            "digest_of": f"all {n} result records of the last timed step, computed on the device; the buffer held a fill pattern before the timed steps",
            "edges": edges, "ambiguous_band_records": n_amb}


def run_workload(workload, order, scaling, args, torch, dist, rank, local_rank, world, with_gather, gather_mode="ring", dump_dir=None):
    """Timed steps + kernel timing of one workload on this rank; returns (record for the JSON line, reads, candidates, settings).
    dump_dir: rank 0 writes what the last timed step computed there (dump_outputs)."""
    import haploconduct_amd as hc
    from haploconduct_amd import parallel
    from haploconduct_amd.records import REC_COMPACT

    strong = scaling == "strong" and world > 1
    # CUs the scoring launches leave to the collective library's kernels while an exchange runs beside them (hc_set_comm_reserve; every
    # exchange is gated on the scoring kernel having taken its CUs): the scoring kernel otherwise holds a workgroup on EVERY CU for its whole
    # duration and a collective's kernels cannot share a CU with one (profiles/r05_coresident.json)
    reserve_cus = max(0, args.reserve_cus) if with_gather else 0
    on_device = not args.full and order == "sfo"  # only --full needs the host's records (parity, stage, baselines)
    reads, cand, cfg, settings = build_workload(workload, 0 if strong else rank, keep=world > 1, on_device=on_device)
    cfg = dict(cfg)
    if world > 1 and dist.get_world_size() != world:  # the collective library must have seen every rank: never report N ranks on fewer
        raise SystemExit(f"bench.py: --gpus {world} but the process group has {dist.get_world_size()} ranks")
    if strong:
        cfg["workload"] = cfg["workload"].replace("candidates per GPU", f"candidates: the ONE set split over {world} ranks (contiguous shards)")
    settings.device = local_rank
    if order == "grouped":
        cand = cand[np.argsort(cand["read1"], kind="stable")]
    elif order == "shuffled":
        cand = cand[np.random.default_rng(5).permutation(cand.size)]
    n_job = len(cand) * (1 if strong else world)  # candidates one step scores over all ranks
    if strong:  # the one candidate set split over the ranks: contiguous, order-preserving shards
        lo, hi = parallel.shard_range(len(cand), rank, world)
        cand, base_index = cand[lo:hi], lo
    else:
        base_index = rank * len(cand)
    n = len(cand)
    sc = hc.EdgeScorer(settings)
    sc.set_reads(reads)
    # hc_cand_rec: the 16 bytes per candidate the stage sends to the device
    d_in = cand.view(torch.uint8).reshape(-1) if on_device else torch.from_numpy(sc.pack_cands(cand).view(np.uint8).reshape(-1)).cuda()
    d_out = torch.empty(n * 24, dtype=torch.uint8, device="cuda")
    if args.full:
        positions, subs = sc.count_positions_device(d_in.data_ptr(), n, REC_COMPACT)
        # parity, untimed half: one launch into a buffer of its own, reduced to a digest on the device
        d_ref = torch.empty(n * 24, dtype=torch.uint8, device="cuda")
        sc.score_cands_device(d_in.data_ptr(), n, d_ref.data_ptr())
        sc.synchronize()
        digest_untimed = device_digest(torch, d_ref, n)
        del d_ref
    else:  # the same untimed first launch, so that what a first launch sets up is not in the warm-up or, with --warmup 0, the timed steps
        sc.score_cands_device(d_in.data_ptr(), n, d_out.data_ptr())
        sc.synchronize()

    # N > 1: every rank scores its shard against a replicated read store; per step, the non-dropped
    # records of every rank are collected on every rank.  The scoring kernel itself appends them (tagged with their
    # global index) to a payload whose row 0 is the count, so the all-gather-v is ONE all-gather over RCCL per step, on
    # a side stream, overlapping the scoring kernel of the next step; nothing synchronises with the host inside a step
    # (parallel.StreamedGather).  An explicit (non-default) stream for the scoring launches: events and the
    # collection's side stream order against it by themselves.
    launch_stream = torch.cuda.Stream()
    torch.cuda.set_stream(launch_stream)
    stream = launch_stream.cuda_stream
    gather = None
    if with_gather:
        sc.score_cands_device(d_in.data_ptr(), n, d_out.data_ptr(), stream)
        torch.cuda.synchronize()
        coll = "cuda" if dist.get_backend() == "nccl" else "cpu"  # small tensors of the bookkeeping collectives (gloo: test runs only)
        kept = torch.tensor([int((((d_out.view(torch.int64).view(-1, 3)[:, 2] >> 60) & 0xF) != 0).sum().item())], device=coll)
        dist.all_reduce(kept, op=dist.ReduceOp.MAX)  # one capacity for all ranks
        cap_rows = int(kept.item()) * 5 // 4 + 1024
        # 24-byte rows (round 6) where the job allows them: every global index below 2^32, no overlap of 2^14 positions and more
        narrow = parallel.rows_fit_narrow(n_job, int(np.diff(reads.seq_off).max())) and os.environ.get("HC_BENCH_ROW_BYTES", "24") != "32"
        reserve_tried = None
        if args.reserve_cus < 0:
            # how many CUs to leave to the exchange's kernels is decided by trying (set-up, before the warm-up; every rank takes the same
            # decision: the slowest rank's step time counts).  Measured on one GPU with stand-in kernels (profiles/r05_coresident.md): beside
            # a scoring kernel that holds every CU the exchange is serialised behind it (step = kernel + exchange); with CUs left free and the
            # gate it overlaps if the exchange's workgroups fit the free CUs — at the price of those CUs for the scoring kernel.  Which is
            # cheaper depends on N (the shard's kernel time against the payload) and on the collective library's kernels.
            reserve_tried = {}
            for r_try in (0, 16, 32):
                g_try = parallel.StreamedGather(sc, n, base_index=base_index, cap_rows=cap_rows, rec_fmt=REC_COMPACT, mode=gather_mode, reserve_cus=r_try,
                                                narrow=narrow)
                for _ in range(2):
                    g_try.score_step(d_in.data_ptr(), d_out)
                g_try.finish()
                dist.barrier()
                t_try = time.perf_counter()
                for _ in range(6):
                    g_try.score_step(d_in.data_ptr(), d_out)
                g_try.finish()
                t_mine = torch.tensor([(time.perf_counter() - t_try) / 6 * 1e3], device=coll, dtype=torch.float64)
                dist.all_reduce(t_mine, op=dist.ReduceOp.MAX)
                reserve_tried[r_try] = float(t_mine.item())
                g_try.close()
                del g_try
            reserve_cus = min(reserve_tried, key=reserve_tried.get)
        gather = parallel.StreamedGather(sc, n, base_index=base_index, cap_rows=cap_rows, rec_fmt=REC_COMPACT, mode=gather_mode, reserve_cus=reserve_cus,
                                         narrow=narrow)
    last = None

    def step():
        nonlocal last
        if gather:  # the scoring kernel appends the collection payload itself; the all-gather of step i runs on a
            last = gather.score_step(d_in.data_ptr(), d_out)  # side stream beside the kernel of step i + 1
        else:
            sc.score_cands_device(d_in.data_ptr(), n, d_out.data_ptr(), stream)

    for _ in range(args.warmup):
        step()
    if gather:
        gather.finish()
        gather.reset_timings()
    sc.synchronize()
    d_out.fill_(0xA5)  # whatever the timed steps leave here, they wrote
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sc.synchronize()
    launch_stream.synchronize()
    t_scored = time.perf_counter()
    if gather:
        gather.finish()  # every all-gather of the timed steps has completed
    torch.cuda.synchronize()
    dt_local = time.perf_counter() - t0
    gather_wait_ms = (time.perf_counter() - t_scored) * 1e3  # what the collection still needed once this rank's kernels were done
    if dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    gather_ms = 0.0
    if gather:  # outside the timed region: the collected set is what it should be
        gather_ms = gather.gather_ms()  # the collective(s) of a step alone: events on the side stream, mean over the timed steps
        rows, counts = gather.collect(last)
        assert len(counts) == world
        if rows is None:  # "root": the rows went to rank 0 and nowhere else
            assert gather_mode == "root" and rank != 0
        else:
            assert rows.shape[0] == sum(counts) and bool((rows[1:, 0] > rows[:-1, 0]).all()), "gathered rows out of order"
        if args.dump_rows and rank == 0:  # tests: the collected rows of the last step, as every rank (root form: rank 0) holds them
            np.save(args.dump_rows, rows.cpu().numpy())
        gather.close()  # the CU reserve goes: the kernel timing below is a whole-device figure (round-5 advisor)
    if dist:
        coll = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([dt], device=coll, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if dump_dir and rank == 0:  # outside the timed region, before anything else launches into d_out
        dump_outputs(torch, d_out, n, dump_dir)
    kern_ms = None
    if args.full:
        # parity, timed half: the digest of what the last timed step left, and stretches of it against the CPU oracle
        parity = parity_record(torch, sc, reads, settings, cand, d_out, n, device_digest(torch, d_out, n), digest_untimed)
        # kernel-only: hipEvents on the stream the kernel is launched on
        # (the parity leg above left the device idle for seconds — CPU oracle — and its clocks down: a few untimed launches first, as the timed
        # steps have their warm-up; round 5's figure carried the ramp: kernel_ms above ms_per_step)
        sc.time_kernel(d_in.data_ptr(), n, d_out.data_ptr(), max(2, min(args.warmup, 5)), REC_COMPACT)
        kern_ms = sc.time_kernel(d_in.data_ptr(), n, d_out.data_ptr(), max(10, min(args.steps, 200)), REC_COMPACT)
        kinfo = sc.kernel_info(n)  # the form a launch of this size takes
        symbytes = 2 if "encoding=u16" in kinfo else 1
    per_rank = None
    if dist:  # what every rank saw, gathered outside the timed region
        mine = torch.tensor([kern_ms or 0.0, dt_local / args.steps * 1e3, gather_wait_ms / max(args.steps, 1), float(dist.get_world_size()), float(n),
                             gather_ms], device=coll, dtype=torch.float64)
        everyone = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(everyone, mine)
        per_rank = [{"rank": r, "kernel_ms": float(v[0]), "step_ms": float(v[1]), "gather_ms": float(v[5]), "gather_wait_ms_per_step": float(v[2]),
                     "n_ranks_seen": int(v[3]), "candidates": int(v[4])} for r, v in enumerate(everyone)]
        if len(per_rank) != world or any(p["n_ranks_seen"] != world for p in per_rank):
            raise SystemExit(f"bench.py: {world} ranks asked for, the collective library reports {[p['n_ranks_seen'] for p in per_rank]}")
        if not args.full:
            for p in per_rank:
                del p["kernel_ms"]
    rec = {
        "value": n_job * args.steps / dt,
        "ms_per_step": dt / args.steps * 1e3,
        "config": dict(cfg, candidates_per_gpu=n, candidates_per_step=n_job, record_bytes=16,
                       parallelism=f"candidate shards x{world}, replicated read store" +
                                   ((", one all-gather of the non-dropped records per step (fixed-capacity payload, the library's ring)" if gather_mode == "ring" else
                                     (", one all-gather-v of the non-dropped records per step (counts, then grouped per-peer send / recv of exactly the rows)"
                                      if gather_mode == "direct" else
                                      ", the non-dropped records of every rank to rank 0 per step (counts by one small all-gather, then one send of exactly the rows per rank)"))
                                    if gather else ""),
                       **({"gather": gather_mode, "gather_row_bytes": 24 if narrow else 32, "reserve_cus": reserve_cus,
                           "reserve_cus_tried_ms_per_step": {str(k): v for k, v in reserve_tried.items()} if reserve_tried else None} if gather else {}),
                       edge_threshold=settings.edge_threshold),
    }
    if args.full:
        rec["config"]["mean_positions_per_candidate"] = positions / max(n, 1)
        rec["roofline"] = roofline_record(workload, order, n, positions, kern_ms, kinfo, symbytes)
        rec["parity"] = parity
    if per_rank:
        rec["ranks"] = {"n_ranks_seen": per_rank[0]["n_ranks_seen"], "gather": gather_mode if gather else None, "per_rank": per_rank,
                        "gather_ms_max": max(p["gather_ms"] for p in per_rank),
                        "gather_ms_is": "the step's collective(s) alone, events on the side stream, mean over the timed steps (it runs beside the next step's kernel)"}
        if args.full:
            # overlap: the share of the all-gather's time hidden behind the scoring kernel = 1 - (step - kernel) / gather alone is not
            # observable without a second run; what is: a step costs step_ms against a kernel of kernel_ms, the difference is what the
            # collection adds on the critical path
            rec["ranks"]["collection_on_critical_path_ms"] = max(0.0, rec["ms_per_step"] - max(p["kernel_ms"] for p in per_rank))
    sc.close()
    del d_in, d_out
    torch.cuda.empty_cache()
    return rec, reads, cand, settings


def stage_end_to_end(reads, cand, settings, threads, reps=4):
    """text overlaps file + FASTQ in -> populated OverlapGraph in sortEdges order + nonedge_overlaps.txt
    out, through the host mirror (hc_ec_open, hc_ec_construct_edges_sorted) on this box; files in a scratch directory."""
    import shutil
    import tempfile

    from haploconduct_amd import host

    d = tempfile.mkdtemp(prefix="hcstage_") + "/"
    try:
        t0 = time.perf_counter()
        host.write_overlaps(d + "overlaps.txt", cand, reads)
        paired = reads.is_paired(0)
        reads.write_fastq(None if paired else d + "singles.fastq", d + "paired1.fastq" if paired else None, d + "paired2.fastq" if paired else None)
        t_files = time.perf_counter() - t0
        settings.n_threads = threads
        kw = dict(singles=None if paired else d + "singles.fastq", paired1=d + "paired1.fastq" if paired else None,
                  paired2=d + "paired2.fastq" if paired else None, overlaps=d + "overlaps.txt", output_dir=d)
        runs = []
        for _ in range(reps):
            if os.path.exists(d + "nonedge_overlaps.txt"):
                os.remove(d + "nonedge_overlaps.txt")
            t0 = time.perf_counter()
            ec = host.EdgeCalculatorStage(settings, **kw)
            t1 = time.perf_counter()
            ec.construct_edges_sorted()
            t2 = time.perf_counter()
            c = ec.counters()
            runs.append({"open_s": t1 - t0, "construct_edges_sorted_s": t2 - t1, "edges": ec.edge_count(), "scored": c["scored"],
                         "parse_s": c["t_parse"], "collect_s": c["t_score"], "resolve_s": c["t_insert"], "write_s": c["t_write"]})
            ec.close()
        by_time = sorted(runs, key=lambda r: r["construct_edges_sorted_s"])
        best, median = by_time[0], by_time[(len(by_time) - 1) // 2]  # lower median: never better than half of the runs
        by_total = sorted(r["open_s"] + r["construct_edges_sorted_s"] for r in runs)
        return {"value": median["scored"] / median["construct_edges_sorted_s"], "unit": "candidate overlaps/s", "threads": threads,
                "value_is": "median run", "best_value": best["scored"] / best["construct_edges_sorted_s"],
                "open_plus_construct_s": {"median": by_total[(len(by_total) - 1) // 2], "best": by_total[0]},
                "text_bytes": os.path.getsize(d + "overlaps.txt"), "files_written_s": t_files, "median": median, "best": best, "runs": runs,
                "what": "hc_ec_construct_edges_sorted: the overlaps file's text -> H2D in 16 MiB blocks -> device: lines, parse, prefilter, "
                        "scoring kernel, non-dropped rows in file order -> host exp() of the admitted -> device duplicate resolution + "
                        "adjacency in sortEdges order -> OverlapGraph; `value` is the MEDIAN of the runs (a process's first call is the "
                        "slowest); FASTQ load + store upload + device warm-up + block allocation (open_s) are not part of it, as in the "
                        "reference's own timing (src/ViralQuasispecies.cpp:280-283) — open_plus_construct_s has them"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def stage_a_from_reads(reads, settings, threads, err=0.0, min_overlap=90, reps=3):
    """Reads -> sorted graph with no overlaps file (the front of SAVAGE stage a: savage.py:643-717 runs rust-overlaps, scripts/sfo2overlaps.py and
    the binary as three programs), by both routes of this library on the workload's own reads: `from_reads` — the SFO ingest's matching on the
    host threads, the overlaps file's text in memory, copied into the device's text blocks and parsed there — and `from_store` (round 6) —
    nothing but device memory in between (hc_ec_construct_edges_from_store).  Candidate generation (hc_find_overlaps) stands in for
    rust-overlaps, which is not in the reference tree: PARITY UNPINNED there; both routes score the same lines, and the graphs must be equal."""
    import shutil
    import tempfile

    from haploconduct_amd import host

    d = tempfile.mkdtemp(prefix="hcstagea_") + "/"
    try:
        paired = reads.is_paired(0)
        reads.write_fastq(None if paired else d + "singles.fastq", d + "paired1.fastq" if paired else None, d + "paired2.fastq" if paired else None)
        settings.n_threads = threads
        kw = dict(singles=None if paired else d + "singles.fastq", paired1=d + "paired1.fastq" if paired else None,
                  paired2=d + "paired2.fastq" if paired else None, output_dir=d)
        res, digest = {}, {}
        host.keep_devices(True)  # a pipeline's iterations in one process: the stages take over each other's devices (contexts, scratch, blocks)
        for route in ("from_reads", "from_store", "from_reads", "from_store"):  # interleaved: a process's first call pays the finder's allocations
            for _ in range(reps if route in res else 1):
                t0 = time.perf_counter()
                with host.EdgeCalculatorStage(settings, **kw) as ec:
                    t_open = time.perf_counter() - t0
                    t1 = time.perf_counter()
                    if route == "from_store":
                        n_found, n_lines, on_device = ec.construct_edges_from_store(err, min_overlap)
                    else:
                        (n_found, n_lines), on_device = ec.construct_edges_from_reads(err, min_overlap), False
                    t_call = time.perf_counter() - t1
                    edges = ec.edges()
                    dg = (int(edges.size), hash(edges.tobytes()), hash(open(d + "nonedge_overlaps.txt", "rb").read()))
                res.setdefault(route, []).append({"open_s": t_open, "call_s": t_call, "sfo_records": int(n_found), "overlap_lines": int(n_lines),
                                                  "edges": dg[0], "lines_stayed_on_device": bool(on_device)})
                digest.setdefault(route, dg)
                if digest[route] != dg:
                    raise SystemExit(f"bench.py: {route} gave two different graphs")
        if digest["from_reads"] != digest["from_store"]:
            raise SystemExit("bench.py: the device-resident stage a built another graph than the text route")
        med = {r: sorted(x["call_s"] for x in v[1:])[len(v[1:]) // 2] for r, v in res.items()}
        last = res["from_store"][-1]
        return {"value": med["from_store"], "unit": "s (reads in the stage's store -> sorted graph, median of the runs behind each route's first)",
                "from_store_s": med["from_store"], "from_reads_s": med["from_reads"], "speedup": med["from_reads"] / med["from_store"],
                "sfo_records": last["sfo_records"], "overlap_lines": last["overlap_lines"], "edges": last["edges"],
                "lines_stayed_on_device": last["lines_stayed_on_device"], "graphs_equal": True, "finder": {"err_rate": err, "min_overlap": min_overlap},
                "runs": {r: [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in x.items()} for x in xs] for r, xs in res.items()},
                "parity": "the two routes build the same graph and nonedge_overlaps.txt (checked here); the text route is pinned against the reference's "
                          "own construct_edges + sortEdges (tests/test_gpu_c3.py); candidate generation: parity UNPINNED (rust-overlaps is absent)"}
    finally:
        host.keep_devices(False)
        shutil.rmtree(d, ignore_errors=True)


def stage_a_from_sfo(reads, settings, threads, err=0.0, min_overlap=90, reps=2):
    """The pipelines' own input to stage a — the SFO file rust-overlaps writes (savage.py:664) — to the sorted graph: ONE call
    (hc_ec_construct_edges_from_sfo: the file's text, scripts/sfo2overlaps.py's ingest and the stage all on the device) against the THREE steps
    the pipeline runs (the script -> original_overlaps.txt -> the binary; here their ports hc_sfo2overlaps + hc_ec_construct_edges_sorted).  The
    SFO file is this library's finder's output on the workload's reads, written once, untimed; from the file on everything is pinned (the ingest
    by the script's own outputs, the stage by the reference's own construct_edges + sortEdges)."""
    import shutil
    import tempfile

    import haploconduct_amd as hc
    from haploconduct_amd import host

    d = tempfile.mkdtemp(prefix="hcsfo_") + "/"
    try:
        paired = reads.is_paired(0)
        reads.write_fastq(None if paired else d + "singles.fastq", d + "paired1.fastq" if paired else None, d + "paired2.fastq" if paired else None)
        settings.n_threads = threads
        fq = dict(singles=None if paired else d + "singles.fastq", paired1=d + "paired1.fastq" if paired else None,
                  paired2=d + "paired2.fastq" if paired else None)
        with hc.EdgeScorer(settings) as sc:
            sc.set_reads(reads)
            recs = sc.find_overlaps(err, min_overlap)
        host.write_sfo(d + "sfoverlaps.out", recs)
        n_rec = int(recs.size)
        del recs
        n_single, n_pairs = (0, reads.n_reads) if paired else (reads.n_reads, 0)
        host.keep_devices(True)
        one, three = [], []
        for _ in range(reps + 1):  # (the first round pays a process's first allocations: not counted)
            with host.EdgeCalculatorStage(settings, output_dir=d, **fq) as ec:
                t0 = time.perf_counter()
                nr, nl, on_device = ec.construct_edges_from_sfo(d + "sfoverlaps.out")
                t1 = time.perf_counter()
                a = (ec.edge_count(), hash(ec.edges().tobytes()), hash(open(d + "nonedge_overlaps.txt", "rb").read()))
            one.append({"s": t1 - t0, "sfo_records": int(nr), "overlap_lines": int(nl), "lines_stayed_on_device": bool(on_device)})
            t0 = time.perf_counter()
            n_lines = host.sfo2overlaps(d + "sfoverlaps.out", d + "original_overlaps.txt", n_single, n_pairs)
            t1 = time.perf_counter()
            with host.EdgeCalculatorStage(settings, output_dir=d, overlaps=d + "original_overlaps.txt", **fq) as ec:
                t2 = time.perf_counter()
                ec.construct_edges_sorted()
                t3 = time.perf_counter()
                b = (ec.edge_count(), hash(ec.edges().tobytes()), hash(open(d + "nonedge_overlaps.txt", "rb").read()))
            if a != b or nl != n_lines:
                raise SystemExit("bench.py: the SFO file in one call built another graph than the three steps")
            three.append({"sfo2overlaps_s": t1 - t0, "construct_edges_sorted_s": t3 - t2, "s": t1 - t0 + t3 - t2})
        med = lambda xs: sorted(xs)[len(xs) // 2]
        return {"value": med([x["s"] for x in one[1:]]), "unit": "s (SFO file -> sorted graph, one call; median of the runs behind the first)",
                "one_call_s": med([x["s"] for x in one[1:]]), "three_steps_s": med([x["s"] for x in three[1:]]),
                "speedup": med([x["s"] for x in three[1:]]) / med([x["s"] for x in one[1:]]), "sfo_records": n_rec,
                "sfo_file_bytes": os.path.getsize(d + "sfoverlaps.out"), "overlap_lines": one[-1]["overlap_lines"], "edges": a[0],
                "lines_stayed_on_device": one[-1]["lines_stayed_on_device"], "graphs_equal": True,
                "runs": {"one_call": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in x.items()} for x in one],
                         "three_steps": [{k: round(v, 4) for k, v in x.items()} for x in three]}}
    finally:
        host.keep_devices(False)
        shutil.rmtree(d, ignore_errors=True)


def summary_record(out, args):
    """The line's figures once more, compact and LAST (the driver's record keeps the tail of stdout)."""
    r = out.get("roofline", {})
    def g(x, nd=5):  # compact: the driver's record keeps 2 000 characters of tail
        return float(f"{x:.{nd}g}") if isinstance(x, float) else x

    sm = {"value": g(out["value"]), "ms_per_step": g(out["ms_per_step"]), "n_gpus": out["n_gpus"], "scaling": out["scaling"], "workload": args.workload}
    if args.full:
        sm.update({"kernel_ms": g(r.get("kernel_ms")), "roofline_frac": g(r.get("frac"), 4), "roofline_bound": r.get("bound"),
                   "roofline_frac_8d_note": "8(d) bytes give %.2f of peak (not a bound: fused symbol byte + L1/L2 reuse); counter traffic gives frac" % (r.get("frac_8d") or 0.0),
                   "parity_checked_records": out.get("parity_checked_records"), "edges": out.get("edges")})
    busy = r.get("busy") or {}
    for k in ("valu", "lds", "ta", "hbm", "lds_bank_conflict_share", "valu_instructions_per_candidate"):
        if k in busy:
            sm["busy_" + k] = round(busy[k], 4)
    st = out.get("stage_end_to_end")
    if st:
        runs = [x["construct_edges_sorted_s"] for x in st["runs"]]
        sm[f"{args.workload}_stage_median_s"], sm[f"{args.workload}_stage_first_s"] = g(st["median"]["construct_edges_sorted_s"], 4), g(runs[0], 4)
        sm[f"{args.workload}_stage_runs_s"] = [round(x, 4) for x in runs]
        sm[f"{args.workload}_stage_lines_per_s"] = g(st["value"], 4)
    sa = out.get("stage_a_from_reads")
    if sa:
        sm[f"{args.workload}_reads_to_graph_from_store_s"], sm[f"{args.workload}_reads_to_graph_from_reads_s"] = g(sa["from_store_s"], 4), g(sa["from_reads_s"], 4)
    ss = out.get("stage_a_from_sfo")
    if ss:
        sm[f"{args.workload}_sfo_file_to_graph_s"], sm[f"{args.workload}_sfo_three_steps_s"] = g(ss["one_call_s"], 4), g(ss["three_steps_s"], 4)
    for w, rec in (out.get("also") or {}).items():
        sm[f"{w}_ms_per_step"], sm[f"{w}_kernel_ms"] = g(rec["ms_per_step"], 4), g(rec["roofline"]["kernel_ms"], 4)
        if rec["roofline"].get("frac") is not None:
            sm[f"{w}_roofline_frac"] = g(rec["roofline"]["frac"], 3)
        if rec.get("stage_end_to_end"):
            sm[f"{w}_stage_median_s"] = g(rec["stage_end_to_end"]["median"]["construct_edges_sorted_s"], 4)
    cb = out.get("cpu_baseline")
    if cb:
        sm["cpu_baseline"] = {"value": g(cb["value"], 4), "cores": cb["cores"], "kind": cb["kind"],
                              "by_threads": {t: round(v["value"]) for t, v in (cb.get("by_threads") or {}).items()}}
        if cb.get("stage"):
            sm["cpu_baseline_stage"] = {"value": g(cb["stage"]["value"], 4), "cores": cb["stage"]["cores"], "us_per_line": g(cb["stage"]["us_per_line"], 4)}
    if out.get("ranks"):
        sm["gather"] = out["ranks"].get("gather")
        sm["gather_ms_max"] = out["ranks"].get("gather_ms_max")
        if args.full:
            sm["collection_on_critical_path_ms"] = out["ranks"]["collection_on_critical_path_ms"]
            sm["kernel_ms_per_rank"] = [round(p["kernel_ms"], 4) for p in out["ranks"]["per_rank"]]
    for k in ("strong", "weak"):
        if k in out:
            sm[k] = {"value": out[k]["value"], "ms_per_step": out[k]["ms_per_step"]}
    if "gather_modes" in out:
        sm["gather_modes"] = {m: ({"value": v["value"], "ms_per_step": v["ms_per_step"], "gather_ms_max": (v.get("ranks") or {}).get("gather_ms_max")}
                                  if "value" in v else v) for m, v in out["gather_modes"].items()}
    return sm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beyond the headline figure: in-run parity, kernel time and roofline, the stage, the CPU "
                         "baselines, the --also workloads and, at N > 1, the other scaling mode; a run without it does only what `value` needs")
    ap.add_argument("--also", default="c2,c3q25,c3q35,c3q35r,c3q60,c3q70",
                    help="--full: further workloads (comma-separated) measured on one GPU and reported under \"also\" ('none' = skip): config 2, and config 3 with "
                         "25 / 35 / 60 / 70 distinct quality values (the LG = 5 kernel, the two wide 8-bit encodings and the 16-bit-symbol kernel at the headline's "
                         "size; c3q35r: the 35 values drawn from the histogram of the reference's POLYTE example reads instead of uniformly)")
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"],
                    help="N > 1: strong (default) = the workload's ONE candidate set is split over the ranks (BASELINE configs[2]); "
                         "weak = every rank scores its own candidate set of the workload's size")
    ap.add_argument("--one-mode", action="store_true", help="N > 1 with --full: measure only --scaling's mode (default: both, the other one under its name)")
    ap.add_argument("--gather", default="all", choices=["ring", "direct", "root", "both", "all"],
                    help="N > 1, the per-step exchange: ring = one all-gather of the fixed-capacity payload; direct = all-gather-v (counts, then "
                         "grouped per-peer send / recv); both (default) = ring first, then the headline's mode again with direct behind a watchdog")
    ap.add_argument("--reserve-cus", type=int, default=-1,
                    help="N > 1: CUs the scoring launches leave free for the exchange's kernels (0 = none, the exchange is not gated either; "
                         "-1 = decided by trying 0, 16 and 32 during set-up)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the result records of the headline workload's last timed step (rank 0's) to DIR/<name>.npy as float64: "
                         f"x1, x2, mm, n, cls and the record positions (index); above {DUMP_SAMPLE} records a fixed, seeded sample of them")
    ap.add_argument("--dump-rows", default=None, help="N > 1 (or HC_BENCH_FORCE_GATHER=1): rank 0 writes the rows collected in the last step to this .npy file")
    ap.add_argument("--no-stage", action="store_true", help="--full: skip the stage end-to-end measurement")
    ap.add_argument("--stage-threads", type=int, default=0, help="--threads of the stage (0 = min(32, hardware threads))")
    ap.add_argument("--order", default="sfo", choices=["sfo", "grouped", "shuffled"],
                    help="candidate order inside the batch: sfo = sorted by (min id, max id) as scripts/sfo2overlaps.py:53 "
                         "writes overlap files (default); grouped = by read1; shuffled = random (experiment knobs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    # stdout carries exactly one line, the JSON record of rank 0.  Libraries underneath write there too (RCCL prints
    # its version banner through C stdio, flushed at exit): park fd 1 on stderr until the record is printed.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: libhcedge has no CPU fallback")
    # HC_BENCH_BACKEND=gloo HC_BENCH_ONE_DEVICE=1 (tests on a one-GPU box: every rank on device 0, the all-gather staged through the host): the
    # N-rank code path — shards, both scaling modes, per-rank records, parity — without N GPUs.  Never set by the driver; the line says so.
    backend = os.environ.get("HC_BENCH_BACKEND", "nccl")
    one_device = os.environ.get("HC_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    # HC_BENCH_FORCE_GATHER=1: run the N > 1 step (payload + all-gather) on a single rank too, to time and test that
    # code path on one GPU; never set by the driver
    with_gather = world > 1 or os.environ.get("HC_BENCH_FORCE_GATHER") == "1"
    if with_gather:
        # the collective library's kernels run on the CUs the scoring launches leave free (hc_set_comm_reserve): no more workgroups than the
        # largest reserve tried has CUs (one per free CU is what fits: profiles/r05_coresident.md)
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "32")
        import torch.distributed as dist

        if world > 1 and backend != "nccl":
            dist.init_process_group(backend)
        elif world > 1:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29655", rank=0, world_size=1,
                                    device_id=torch.device("cuda", local_rank))

    scaling = args.scaling or ("strong" if world > 1 else "weak")
    from haploconduct_amd.parallel import GATHER_MODES

    modes = list(GATHER_MODES) if args.gather in ("both", "all") else [args.gather]
    main_rec, reads, cand, settings = run_workload(args.workload, args.order, scaling, args, torch, dist, rank, local_rank, world, with_gather, modes[0],
                                                   dump_dir=args.dump_outputs)
    out = None

    def leg_record(rec, mode_name):
        return {"value": rec["value"], "unit": "candidate overlaps/s", "ms_per_step": rec["ms_per_step"], "scaling": mode_name,
                "gather": rec["config"].get("gather"), "gather_row_bytes": rec["config"].get("gather_row_bytes"), "candidates_per_step": rec["config"]["candidates_per_step"],
                "candidates_per_gpu": rec["config"]["candidates_per_gpu"], "kernel_ms": rec.get("roofline", {}).get("kernel_ms"), "ranks": rec.get("ranks"),
                "parity": rec.get("parity")}

    def headline(rec):
        h = {
            "metric": "candidate overlaps scored/sec (edge-calc scoring pass: compute_overlap + overlap_score + admission class, candidates resident in HBM; the whole stage from the overlaps text: stage_end_to_end)",
            "value": rec["value"],
            "unit": "candidate overlaps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": rec["ms_per_step"],
            "higher_is_better": True,
            "scaling": scaling if world > 1 else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": dict(rec["config"], **({"test_run": f"backend {backend}, every rank on one device: NOT a multi-GPU measurement"}
                                             if (backend != "nccl" or one_device) else {})),
        }
        if args.full:
            h.update(roofline=rec["roofline"], parity=rec["parity"], parity_checked_records=rec["parity"]["parity_checked_records"],
                     edges=rec["parity"]["edges"])
        if "ranks" in rec:
            h["ranks"] = rec["ranks"]
        return h

    if rank == 0:
        out = headline(main_rec)
    if dist:
        dist.barrier()
    if world > 1 and args.full and not args.one_mode:
        # the other scaling mode in the same line, so that one driver pass over N = 1, 2, 4, 8 yields both curves.  The HEADLINE (round 5) is
        # "strong": the ONE candidate set of the workload (BASELINE configs[2]: 1e8 candidates, 1 -> 8 GPUs) split over the ranks — what the
        # north star's "scaling at 8 GPUs" is quoted on; "weak" = every rank its own set.  Same steps, collection, barriers, max-over-ranks clock.
        other = "strong" if scaling == "weak" else "weak"
        del reads, cand
        other_rec, reads, cand, settings = run_workload(args.workload, args.order, other, args, torch, dist, rank, local_rank, world, with_gather, modes[0])
        if rank == 0:
            out[other] = leg_record(other_rec, other)
        dist.barrier()
    if world > 1 and len(modes) > 1:
        # the headline's scaling mode once more with every other form of the exchange, each behind a watchdog: a leg that does not come back (a
        # form of the collective that has never run on this box's fabric) must not cost the line — every rank leaves after `leg_timeout`
        # seconds, rank 0 printing what it has.  The fastest completed leg takes the headline; all are reported under "gather_modes".
        import threading

        leg_timeout = float(os.environ.get("HC_BENCH_LEG_TIMEOUT", "420"))
        legs = {modes[0]: leg_record(main_rec, scaling)} if rank == 0 else {}
        best_rec = main_rec
        for mode in modes[1:]:
            def give_up(why=None, mode=mode):
                if rank == 0:
                    legs[mode] = {"failed": why or f"did not complete within {leg_timeout:.0f} s"}
                    out["gather_modes"] = legs
                    out["summary"] = summary_record(out, args)
                    os.write(real_stdout, (json.dumps(out) + "\n").encode())
                os._exit(0)

            dog = threading.Timer(leg_timeout, give_up)
            dog.daemon = True
            dog.start()
            del reads, cand
            try:
                leg, reads, cand, settings = run_workload(args.workload, args.order, scaling, args, torch, dist, rank, local_rank, world, with_gather, mode)
            except Exception as e:  # (a SystemExit — a parity failure — is not caught: that is a wrong result, not a slow one)
                sys.stderr.write(f"bench.py rank {rank}: the {mode} leg failed: {e!r}\n")
                give_up(repr(e))  # the other ranks may be inside a collective this rank has left: nobody waits for anybody, rank 0 prints what it has
            dog.cancel()
            if rank == 0:
                legs[mode] = leg_record(leg, scaling)
                if leg["value"] > best_rec["value"]:
                    best_rec = leg
            dist.barrier()
        if rank == 0:
            if best_rec is not main_rec:
                extras = {k: v for k, v in out.items() if k in ("strong", "weak")}
                out = dict(headline(best_rec), **extras)
            out["gather_modes"] = legs
            out["gather_modes_note"] = (f"`value` is the fastest of the forms of the per-step exchange ({out['config'].get('gather')}), each a full leg of "
                                        f"{args.steps} timed steps with its own warm-up and barriers" + (" and in-run parity" if args.full else ""))
        dist.barrier()
    if rank == 0 and world == 1 and args.full:
        if not args.no_stage:
            threads = args.stage_threads or min(32, os.cpu_count() or 1)
            out["stage_end_to_end"] = stage_end_to_end(reads, cand, settings, threads)
            out["stage_a_from_reads"] = stage_a_from_reads(reads, settings, threads)
            out["stage_a_from_sfo"] = stage_a_from_sfo(reads, settings, threads)
        if not args.no_cpu_baseline:
            # the reference's own code where its probe library is present (it is built by __graft_entry__.build() in the
            # build container and travels with the repository), and always the oracle (a port) beside it
            port = cpu_baseline(reads, settings, cand)
            genuine = cpu_baseline_reference(reads, settings, cand)
            out["cpu_baseline"] = genuine if genuine else port
            if genuine:
                out["cpu_baseline_port"] = port
                # the reference's stage = its serial text parser + process_overlaps + sortEdges: measured on this box (round 3 estimated
                # it from a per-line figure taken on another machine)
                out["cpu_baseline"]["stage"] = cpu_baseline_stage_reference(reads, settings, cand)
        del reads, cand
        also = [w for w in (args.also or "").split(",") if w and w not in ("none", args.workload)]
        for w in also:
            also_rec, r2, c2, s2 = run_workload(w, args.order, "weak", args, torch, None, 0, local_rank, 1, False)
            if not args.no_stage and c2.size <= 4000000:  # (the stage of the 10^8-candidate variants: the headline workload's own record)
                also_rec["stage_end_to_end"] = stage_end_to_end(r2, c2, s2, args.stage_threads or min(32, os.cpu_count() or 1), reps=3)
            out.setdefault("also", {})[w] = also_rec
            del r2, c2
        if out.get("also"):
            # the quality alphabets real reads have, at the headline's size (round 6): every variant's kernel, time, roofline position and
            # its per-position rate against the headline kernel's — inside `roofline`, which a record that keeps the main keys keeps whole
            head_rate = out["roofline"].get("kernel_positions_per_s") or 0.0
            out["roofline"]["alphabets"] = {
                w: {"quality_alphabet": rec["config"].get("quality_alphabet"), "kernel": rec["roofline"]["kernel"], "kernel_ms": rec["roofline"]["kernel_ms"],
                    "ms_per_step": rec["ms_per_step"], "positions_per_s": rec["roofline"]["kernel_positions_per_s"],
                    "rate_vs_headline_kernel": (rec["roofline"]["kernel_positions_per_s"] / head_rate) if head_rate else None,
                    "frac": rec["roofline"].get("frac"), "bound": rec["roofline"].get("bound"), "traffic": rec["roofline"].get("traffic"),
                    "busy": {k: round(v, 4) for k, v in (rec["roofline"].get("busy") or {}).items() if k != "kernel_cycles"},
                    "parity_checked_records": rec["parity"]["parity_checked_records"]}
                for w, rec in out["also"].items()}
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    sys.stdout.flush()
    ctypes.CDLL(None).fflush(None)  # whatever C stdio still holds goes to stderr
    os.dup2(real_stdout, 1)
    os.close(real_stdout)
    if rank == 0:
        # the compact summary right behind the contract's keys AND last in the line: a record that keeps the head, the main keys or only the
        # tail of stdout keeps it (round 6)
        sm = summary_record(out, args)
        first = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
        line = {k: out[k] for k in first if k in out}
        line["summary_first"] = sm
        line.update({k: v for k, v in out.items() if k not in line})
        line["summary"] = sm
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
