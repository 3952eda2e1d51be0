"""Shared by the removeTips / removeBranches tests: the cases of tests/golden/tips_branches.json as graphs and read tables,
the host mirror's and the device's runs of a variant, and read tables for seeded graphs."""
import json
import os

import numpy as np

from haploconduct_amd.host import EDGE_DTYPE, READ_GEOM_DTYPE
from tests import _trans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tips_branches.json")
VARIANTS = {"tips": ("tips",), "branches": ("branches",), "tips_branches": ("tips", "branches")}
TIP_KEYS = ("out_tip_count", "tip_count")
BRANCH_KEYS = ("transitive_kept", "n_out_branch", "n_in_branch", "n_components", "n_tied_lists")


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def golden_records(edges_in):
    """The full records of a case's input edges (the encoding of make_golden_tips.py)."""
    r = np.zeros(len(edges_in), EDGE_DTYPE)
    for k, (v1, v2, r1, r2, p1, p2, l1, l2, o1, o2, od) in enumerate(edges_in):
        r[k] = (1.0, 0.0, p1, p2, -3, k, o1, o2, od, 0, r1, r2, 0, v1, v2, 100, l1 + l2, l1, l2)
    return r


def read_geom(reads):
    g = np.zeros(len(reads), READ_GEOM_DTYPE)
    for k, (l1, l2, p) in enumerate(reads):
        g[k]["len1"], g[k]["len2"], g[k]["paired"] = l1, l2, p
    return g


def run_steps(obj, steps, max_tip_len, geom, device):
    """The steps on a loaded EdgeScorer (device) or an adopted HostGraph; returns {step: counts}."""
    counts = {}
    for st in steps:
        if st == "tips":
            counts[st] = obj.graph_remove_tips(max_tip_len, geom) if device else obj.remove_tips(max_tip_len, geom)
        elif st == "branches":
            counts[st] = obj.graph_remove_branches() if device else obj.remove_branches()
        elif st == "inclusions":
            counts[st] = obj.graph_remove_inclusions() if device else obj.remove_inclusions()
        elif st == "transitive":
            counts[st] = obj.graph_remove_transitive(1, False) if device else obj.remove_transitive_edges(1, False)
    return counts


def mirror_run(edges, out_off, in_nodes, in_off, steps, max_tip_len, geom, incl=None):
    m = _trans.Mirror(edges, out_off, in_nodes, in_off, incl)
    counts = run_steps(m.g, steps, max_tip_len, geom, False)
    out, ioff, inodes = m.result()
    return dict(edges=out, in_off=ioff, in_nodes=inodes.astype(np.uint32), branching=m.g.branching_edges(), tips=m.g.tip_reads(len(geom)),
                counts=counts)


def device_run(sc, edges, out_off, in_nodes, in_off, steps, max_tip_len, geom, incl=None):
    sc.graph_load(edges, out_off, in_nodes, in_off, incl)
    counts = run_steps(sc, steps, max_tip_len, geom, True)
    got = sc.graph_fetch()
    got.update(branching=sc.graph_branching_edges(), tips=sc.graph_tip_reads(len(geom)), counts=counts)
    return got


def check_counts(counts, var, where):
    """The counters of a golden variant against hc_tip_counts / hc_branch_counts."""
    if "tips" in counts:
        for k in TIP_KEYS:
            assert counts["tips"][k] == var[k], (where, k, counts["tips"], var[k])
        assert counts["tips"]["n_tip_reads"] == sum(var["tip_reads"]), where
        assert counts["tips"]["edges_before"] - counts["tips"]["n_removed"] == counts["tips"]["edges_after"], where
    if "branches" in counts:
        for k in BRANCH_KEYS:
            assert counts["branches"][k] == var[k], (where, k, counts["branches"], var[k])
        assert counts["branches"]["n_removed"] == var["n_removed_branches"], where
        assert counts["branches"]["edges_after"] == var["edge_count"], where
    last = counts["branches"] if "branches" in counts else counts["tips"]
    assert last["edges_after"] == var["edge_count"], where
    assert sum(c["n_removed"] for c in counts.values()) == len(var["branching"]), where


def tip_geometry(edges, V, n_reads, seed, frac=0.1):
    """A read table for a seeded graph over single-end reads: the records get pos1 / len1 such that about `frac` of the
    edges into dead ends (and out of sources) extend by fewer than 150 bases, a few of them by none; the rest by more."""
    rng = np.random.default_rng(seed)
    geom = np.zeros(n_reads, READ_GEOM_DTYPE)
    geom["len1"] = 250
    e = edges.copy()
    n = e.shape[0]
    kind = rng.random(n)
    ext = np.where(kind < frac / 4, 0, np.where(kind < frac, rng.integers(1, 150, n), rng.integers(150, 240, n))).astype(np.int32)
    e["len1"], e["len2"] = 250 - ext, 0       # S-S forward: ext_len(1) = 250 - len0
    e["len0"] = e["len1"]
    e["pos1"], e["pos2"] = ext, 0             # backward: ext_len(0) = pos1 + pos2
    return e, geom
