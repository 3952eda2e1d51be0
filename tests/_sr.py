"""Shared by the super-read consensus tests: the golden file as a ReadSet + layouts, and layout generators."""
import json
import os

import numpy as np

from haploconduct_amd import consensus as SR
from haploconduct_amd.readstore import ReadSet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consensus.json")


def load_golden():
    """-> (reads, cases, read_index): the JSON's reads as a ReadSet (singles first, then pairs: m_read_vec order) and the map from the
    JSON's read number to the set's."""
    g = json.load(open(GOLDEN))
    singles = [(i, r) for i, r in enumerate(g["reads"]) if len(r) == 1]
    pairs = [(i, r) for i, r in enumerate(g["reads"]) if len(r) == 2]
    index = {}
    for k, (i, _) in enumerate(singles + pairs):
        index[i] = k
    reads = ReadSet.from_lists([tuple(r[0]) for _, r in singles], [(tuple(r[0]), tuple(r[1])) for _, r in pairs])
    return reads, g["cases"], index


def case_arrays(cases, index):
    """All cases of one settings tuple as one batch: -> (layouts, members)."""
    n_m = sum(len(c["members"]) for c in cases)
    layouts = np.zeros(len(cases), SR.SR_LAYOUT_DTYPE)
    members = np.zeros(n_m, SR.SR_MEMBER_DTYPE)
    k = 0
    for i, c in enumerate(cases):
        layouts[i] = (k, len(c["members"]), c["total_len"])
        for m in c["members"]:
            members[k] = (index[m["read"]], m["pos"], m["seq"], m["rev"], (0, 0))
            k += 1
    return layouts, members


def by_settings(cases):
    groups = {}
    for c in cases:
        s = c["settings"]
        groups.setdefault((s["min_qual"], s["min_clique_size"], s["error_correction"], s["subreads_needed"]), []).append(c)
    return groups


def check_against_golden(run):
    """run(layouts, members, min_qual, min_clique_size, error_correction, subreads_needed) -> SrResult; compares every golden case."""
    reads, cases, index = load_golden()
    n = 0
    for key, group in sorted(by_settings(cases).items()):
        layouts, members = case_arrays(group, index)
        res = run(reads, layouts, members, *key)
        for i, c in enumerate(group):
            seq, qual = res.seq(i)
            assert int(res.ret[i]) == c["ret"], (c["name"], int(res.ret[i]), c["ret"])
            assert seq.decode() == c["cons_seq"], (c["name"], seq, c["cons_seq"])
            assert qual.decode() == c["cons_qual"], (c["name"], qual, c["cons_qual"])
            if c["status"] >= 0:
                assert int(res.status[i]) == c["status"], (c["name"], int(res.status[i]), c["status"])
            else:  # empty with return value 0: the reference does not say which exit it took
                assert int(res.status[i]) in (SR.SR_MEMBER_SHORT, SR.SR_UNCOVERED), c["name"]
            n += 1
    return n


def random_cliques(rng, reads, n_layouts, depth_lo, depth_hi, single_only=False):
    """Random layouts over the reads of a set: depth in [depth_lo, depth_hi], ascending positions with steps smaller than the
    shortest member (no gaps), both orientations, mates of pairs where the set has them."""
    first = reads.read_first_seq.astype(np.int64)
    paired = (first[1:] - first[:-1]) == 2
    seq_len = (reads.seq_off[1:] - reads.seq_off[:-1]).astype(np.int64)
    depth = rng.integers(depth_lo, depth_hi + 1, n_layouts)
    n_m = int(depth.sum())
    members = np.zeros(n_m, SR.SR_MEMBER_DTYPE)
    cand = np.flatnonzero(~paired) if single_only else np.arange(reads.n_reads)
    r = cand[rng.integers(0, cand.size, n_m)]
    mate = np.where(paired[r], rng.integers(1, 3, n_m), 0)
    members["read"], members["seq"], members["rev"] = r, mate, rng.integers(0, 2, n_m)
    mlen = seq_len[first[r] + (mate == 2)]
    step = rng.integers(0, np.maximum(1, np.minimum(mlen, 24)), n_m)
    start = np.zeros(n_layouts + 1, np.int64)
    start[1:] = np.cumsum(depth)
    step[start[:-1]] = 0
    cum = np.cumsum(step)
    pos = cum - np.repeat(cum[start[:-1]], depth)
    members["pos"] = pos
    # a member may not reach past the previous one's end + 1 without a gap: steps < 24 <= lengths keep the tiling closed for the
    # read sets used here; where they do not, the layout is still well-formed and both sides must report the uncovered column
    layouts = np.zeros(n_layouts, SR.SR_LAYOUT_DTYPE)
    layouts["first_member"], layouts["n_members"] = start[:-1], depth
    layouts["total_len"] = np.maximum.reduceat(pos + mlen, start[:-1])
    return layouts, members


def assert_same(a, b, what=""):
    assert np.array_equal(a.ret, b.ret), what + ": return values differ"
    assert np.array_equal(a.status, b.status), what + ": statuses differ"
    assert np.array_equal(a.out_off, b.out_off), what + ": offsets differ"
    assert np.array_equal(a.cons_seq, b.cons_seq), what + ": cons_seq differs"
    assert np.array_equal(a.cons_qual, b.cons_qual), what + ": cons_qual differs"
