"""Shared by the edge-merge tests: the cases of tests/golden/edge_merge.json as CSR graphs and read sets, the golden layouts as
arrays, and a seeded graph over reads cut from one template."""
import json
import os

import numpy as np

from haploconduct_amd import consensus as SR
from haploconduct_amd.host import EDGE_DTYPE
from haploconduct_amd.readstore import ReadSet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_merge.json")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def csr(V, rows):
    """rows: (v1, v2, read1, read2, pos1, pos2, ori1, ori2, ord) in addEdge order -> (edges, out_off, in_nodes, in_off)."""
    rows = np.asarray(rows, np.int64).reshape(-1, 9)
    order = np.argsort(rows[:, 0], kind="stable")
    e = np.zeros(rows.shape[0], EDGE_DTYPE)
    r = rows[order]
    e["v1"], e["v2"], e["read1"], e["read2"], e["pos1"], e["pos2"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5]
    e["ori1"], e["ori2"], e["ord"] = r[:, 6], r[:, 7], r[:, 8]
    e["score"], e["perc"] = 1.0, 100
    out_off = np.zeros(V + 1, np.uint64)
    out_off[1:] = np.cumsum(np.bincount(rows[:, 0], minlength=V))
    in_order = np.argsort(rows[:, 1], kind="stable")  # adj_in[w] in insertion order
    in_nodes = rows[in_order, 0].astype(np.uint32)
    in_off = np.zeros(V + 1, np.uint64)
    in_off[1:] = np.cumsum(np.bincount(rows[:, 1], minlength=V))
    return e, out_off, in_nodes, in_off


def random_reads(lens, seed, quals=(40, 70)):
    """A ReadSet with the given [len1, len2, paired] per read, in that order."""
    rng = np.random.default_rng(seed)
    seq_len, first = [], [0]
    for l1, l2, p in lens:
        seq_len += [l1, l2] if p else [l1]
        first.append(len(seq_len))
    off = np.zeros(len(seq_len) + 1, np.uint64)
    off[1:] = np.cumsum(seq_len)
    total = int(off[-1])
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total)]
    q = rng.integers(quals[0], quals[1], total).astype(np.uint8)
    return ReadSet(bases, q, off, np.asarray(first, np.uint32), np.arange(len(lens), dtype=np.uint64))


def golden_arrays(case):
    """The golden layouts of a case as hc_sr_edge_merge packs them: (pairs, first_layout, layouts, members)."""
    pairs = np.asarray([p["pair"] for p in case["pairs"]], np.uint32).reshape(-1, 2)
    first, lay, mem = [0], [], []
    for p in case["pairs"]:
        for total, lst in zip(p["total_len"], p["lists"]):
            lay.append((len(mem), len(lst), total))
            mem += [(read, pos, seq, rev, (0, 0)) for read, seq, rev, pos, _ in lst]
        first.append(len(lay))
    return pairs, np.asarray(first, np.uint64), np.asarray(lay, SR.SR_LAYOUT_DTYPE), np.asarray(mem, SR.SR_MEMBER_DTYPE)


def assert_layouts(got, first, layouts, members, what):
    """Every pair laid out, and the packed layouts and members equal."""
    assert (got.pair_status == SR.SR_EDGE_OK).all(), (what, got.pair_status)
    assert np.array_equal(got.first_layout, first), what + ": first_layout differs"
    assert np.array_equal(got.layouts, layouts), what + ": layouts differ"
    assert np.array_equal(got.members, members), what + ": members differ"


def planted():
    """Reads 0-1 single-end, 2-4 paired; vertex v reads read v; vertex 5 names a read beyond the store."""
    lens = [[50, 0, 0], [60, 0, 0], [50, 40, 1], [45, 45, 1], [70, 30, 1]]
    rows = [[0, 1, 0, 1, 5, 0, 1, 1, ord("-")],          # fine
            [0, 2, 0, 2, 5, -4, 1, 1, ord("-")],         # mate 2 of a paired member at a negative position
            [2, 3, 0, 1, 5, 0, 1, 1, ord("1")],          # neither read is the base's
            [3, 4, 3, 1, 5, 6, 1, 1, ord("1")],          # a paired layout whose record names a single-end read for the other vertex
            [1, 4, 1, 9, 5, 6, 1, 1, ord("1")],          # the record's other read is beyond the store
            [1, 3, 1, 3, 2**31 - 1, 2**31 - 1, 1, 1, ord("1")]]  # total_len beyond int
    case = dict(V=6, edges_in=rows, reads=lens, vertex_read=[0, 1, 2, 3, 4, 77], vertex_fwd=[1] * 6)
    pairs = [[0, 1], [0, 2], [2, 3], [3, 4], [1, 4], [1, 3], [0, 3], [0, 0], [0, 6], [0, 5], [1, 0]]
    want = [SR.SR_EDGE_OK, SR.SR_EDGE_PAIRED_NEG_POS, SR.SR_EDGE_READ_MISMATCH, SR.SR_EDGE_READ_MISMATCH, SR.SR_EDGE_BAD_VERTEX,
            SR.SR_EDGE_BAD_GEOMETRY, SR.SR_EDGE_NO_EDGE, SR.SR_EDGE_BAD_VERTEX, SR.SR_EDGE_BAD_VERTEX, SR.SR_EDGE_BAD_VERTEX, SR.SR_EDGE_OK]
    return case, pairs, want


def seeded_graph(seed=5, n_reads=2000, template_len=30000, long_lists=(63, 64, 65, 200), quals=(50, 74)):
    """Reads cut from one template (single-end 90-150 bases, or pairs of two such mates 61-89 bases apart), one forward
    vertex per read, and records between reads whose placements agree with the template: pos1 / pos2 are the placements' differences,
    so that every layout is consistent and its consensus succeeds.  Some reads are stored reverse-complemented (vertex_fwd = 0
    restores them).  Hub vertices own out-lists of `long_lists` records with the wanted target last; one pair has its record only
    in the reverse list; some pairs are repeated in a list.  quals: the range of the quality bytes, which decides the store's encoding.
    -> dict(reads, V, rows, vertex_read, vertex_fwd, pairs)."""
    rng = np.random.default_rng(seed)
    tmpl = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, template_len)]
    bases, qual_parts, seq_len, first, place, fwd = [], [], [], [0], [], []

    def cut(a, n, rc):
        s = tmpl[a:a + n]
        if rc:
            s = np.frombuffer(s.tobytes().translate(COMP), np.uint8)[::-1]
        bases.append(s)
        qual_parts.append(rng.integers(quals[0], quals[1], n).astype(np.uint8))
        seq_len.append(n)

    starts = np.sort(rng.integers(0, template_len - 700, n_reads))
    for r in range(n_reads):
        a, paired, f = int(starts[r]), rng.random() < 0.5, rng.random() < 0.7
        l1, l2 = int(rng.integers(90, 151)), int(rng.integers(90, 151))
        gap = int(rng.integers(61, 90))
        if not paired:
            cut(a, l1, not f)
            place.append((a, l1, None, None))
        elif f:  # the forward vertex reads mate 1 at a, mate 2 at a + gap
            cut(a, l1, False)
            cut(a + gap, l2, False)
            place.append((a, l1, a + gap, l2))
        else:    # stored reversed: get_rev_comp(2) lies at a, get_rev_comp(1) at a + gap
            cut(a + gap, l2, True)
            cut(a, l1, True)
            place.append((a, l1, a + gap, l2))
        first.append(len(seq_len))
        fwd.append(1 if f else 0)
    off = np.zeros(len(seq_len) + 1, np.uint64)
    off[1:] = np.cumsum(seq_len)
    reads = ReadSet(np.concatenate(bases), np.concatenate(qual_parts), off, np.asarray(first, np.uint32), np.arange(n_reads, dtype=np.uint64))
    paired = [p[2] is not None for p in place]

    def record(v1, v2):
        """v1 -> v2 with read1 = v1's read: pos1 = left placement of v2 minus that of v1; pos2 likewise for the right mates (a single-end
        read's only sequence stands for both); ord '1'."""
        a1, _, b1, _ = place[v1]
        a2, _, b2, _ = place[v2]
        pos1 = a2 - a1
        if paired[v1] and paired[v2]:
            pos2 = b2 - b1
        elif paired[v2]:
            pos2 = b2 - a1   # mate 2 of the paired read against the single-end base, whichever way the record points (new_pos = pos2, :181)
        elif paired[v1]:
            pos2 = b1 - a2
        else:
            pos2 = 0
        return [v1, v2, v1, v2, pos1, pos2, fwd[v1], fwd[v2], ord("1")]

    rows, pairs = [], []
    hubs = {10 + 40 * k: (n_list, False) for k, n_list in enumerate(long_lists)}  # filler records to far-away vertices, the wanted one last
    hubs[10 + 40 * len(long_lists)] = (100, True)                                  # a long list, the wanted record only in the reverse list
    v = 0
    while v + 1 < n_reads:
        w = v + 1
        if v not in hubs and (w in hubs or place[w][0] - place[v][0] >= 60 or rng.random() > 0.35):
            v += 1
            continue
        kind = rng.random()
        if v in hubs:
            n_list, reverse_only = hubs[v]
            fill = rng.choice(np.arange(n_reads // 2, n_reads), n_list - (0 if reverse_only else 1), replace=False)
            rows += [record(v, int(t)) for t in fill]
            kind = 0.7 if reverse_only else 0.0
        if kind < 0.6:
            rows.append(record(v, w))
        elif kind < 0.8:  # only in the reverse list
            rows.append(record(w, v))
        else:             # repeated, the first wins
            rows.append(record(v, w))
            again = record(v, w)
            again[4] += 3
            rows.append(again)
        pairs.append([v, w] if rng.random() < 0.5 else [w, v])
        v += 2
    return dict(reads=reads, V=n_reads, rows=rows, vertex_read=np.arange(n_reads, dtype=np.uint32), vertex_fwd=np.asarray(fwd, np.uint8),
                pairs=np.asarray(pairs, np.uint32))
