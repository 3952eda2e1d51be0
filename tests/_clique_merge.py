"""Shared by the clique-merge tests: tests/golden/clique_merge.json as a CSR graph, a read set and expected arrays, and a seeded graph of
cliques around base vertices (only base - member records are needed, so the graph stays small)."""
import json
import os

import numpy as np

from haploconduct_amd import consensus as SR

from tests._edge_merge import csr, random_reads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clique_merge.json")
MS = (1, 2, 4)  # the golden cliques' min_clique_size values; one call per (m, ec)


def load_golden():
    """The file with its compact forms spelled out: V, vertex_read (the identity) and edges_in as tests/_edge_merge.py: csr takes them."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    fwd = doc["vertex_fwd"]
    doc["V"] = len(fwd)
    doc["vertex_read"] = list(range(len(fwd)))
    doc["edges_in"] = [[v1, v2, v2 if sw else v1, v1 if sw else v2, p1, p2, fwd[v1], fwd[v2], od] for v1, v2, p1, p2, od, sw in doc["edges"]]
    return doc


def golden_groups(doc):
    """{(m, ec): [clique, ...]}: the cliques that one call (one hc_sr_settings) lays out."""
    groups = {}
    for q in doc["cliques"]:
        groups.setdefault((q["m"], q["ec"]), []).append(q)
    return groups


def golden_arrays(cliques):
    """The golden cliques as hc_sr_clique_merge packs them: (clique_off, clique_nodes, first_layout, layouts, members, member_vertex,
    member_used, trims per layout, subreads)."""
    off, nodes = SR.clique_csr([q["clique"] for q in cliques])
    first, lay, mem, vert, used, trim, sub = [0], [], [], [], [], [], []
    for q in cliques:
        for k, (total, lst) in enumerate(zip(q["total_len"], q["lists"])):
            lay.append((len(mem), len(lst), total))
            mem += [(read, pos, seq, rev, (0, 0)) for read, seq, rev, pos, _, _ in lst]
            vert += [e[4] for e in lst]
            used += [e[5] for e in lst]
            trim.append(q["trim"][k])
        first.append(len(lay))
        sub += [tuple(s) for s in q["subreads"]]
    return (off, nodes, np.asarray(first, np.uint64), np.asarray(lay, SR.SR_LAYOUT_DTYPE), np.asarray(mem, SR.SR_MEMBER_DTYPE),
            np.asarray(vert, np.uint32), np.asarray(used, np.uint8), np.asarray(trim, np.int32), np.asarray(sub, SR.SR_SUBREAD_DTYPE))


def assert_equal_layouts(got, want, what, subreads=True):
    """got: an SrCliqueLayouts; want: golden_arrays' tuple or another SrCliqueLayouts."""
    if isinstance(want, SR.SrCliqueLayouts):
        first, lay, mem, vert, used, sub = want.first_layout, want.layouts, want.members, want.member_vertex, want.member_used, want.subreads
        assert np.array_equal(got.clique_status, want.clique_status), what + ": clique_status differs"
        assert np.array_equal(got.layout_filter, want.layout_filter), what + ": layout_filter differs"
    else:
        _, _, first, lay, mem, vert, used, _, sub = want
        assert (got.clique_status == SR.SR_EDGE_OK).all(), (what, got.clique_status)
    assert np.array_equal(got.first_layout, first), what + ": first_layout differs"
    assert np.array_equal(got.layouts, lay), what + ": layouts differ"
    assert np.array_equal(got.members, mem), what + ": members differ"
    assert np.array_equal(got.member_vertex, vert), what + ": member_vertex differs"
    assert np.array_equal(got.member_used, used), what + ": member_used differs"
    if subreads:
        assert np.array_equal(got.subreads, sub), what + ": subread infos differ"


def golden_graph(doc, seed=3):
    """(edges, out_off, reads) of the golden file: the records in addEdge order as a CSR, random reads of the golden lengths."""
    e, out_off, _, _ = csr(doc["V"], doc["edges_in"])
    return e, out_off, random_reads(doc["reads"], seed)


def seeded_cliques(seed=9, m=4, quals=(50, 74)):
    """About 600 vertices and 150 cliques for min_clique_size m = 4.  Reads are cut from one template, so that every layout is consistent and
    its consensus succeeds; vertex v reads read v.  Clique sizes 2, 3, 12, 13, 16, 17, 40 and single-end cliques of 63 / 64 / 65 vertices;
    bases with lists of 63 / 64 / 65 / 200 records not in target order; repeated base -> node records (the first in list order wins); records
    only in the member's list; one clique per failing status.
    -> dict(reads, V, rows, vertex_read, vertex_fwd, cliques, want_status)."""
    from haploconduct_amd.readstore import ReadSet

    from tests._edge_merge import COMP

    rng = np.random.default_rng(seed)
    template_len = 6000
    tmpl = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, template_len)]
    bases, qual_parts, seq_len, first, place, fwd = [], [], [], [0], [], []

    def cut(a, n, rc):
        s = tmpl[a:a + n]
        if rc:
            s = np.frombuffer(s.tobytes().translate(COMP), np.uint8)[::-1]
        bases.append(s)
        qual_parts.append(rng.integers(quals[0], quals[1], n).astype(np.uint8))
        seq_len.append(n)

    def vertex(a, paired, f=None, l1=None):
        """A read placed at template offset a (mate 2 at a + gap)."""
        f = rng.random() < 0.7 if f is None else f
        l1 = int(rng.integers(90, 131)) if l1 is None else l1
        l2, gap = int(rng.integers(90, 131)), int(rng.integers(61, 90))
        if not paired:
            cut(a, l1, not f)
            place.append((a, l1, None, None))
        elif f:
            cut(a, l1, False)
            cut(a + gap, l2, False)
            place.append((a, l1, a + gap, l2))
        else:  # stored reversed: get_rev_comp(2) lies at a, get_rev_comp(1) at a + gap
            cut(a + gap, l2, True)
            cut(a, l1, True)
            place.append((a, l1, a + gap, l2))
        first.append(len(seq_len))
        fwd.append(1 if f else 0)
        return len(fwd) - 1

    def record(v1, v2, shift=0):
        """v1 -> v2 with read1 = v1's read, as tests/_edge_merge.py: seeded_graph builds it."""
        a1, _, b1, _ = place[v1]
        a2, _, b2, _ = place[v2]
        p1, p2 = place[v1][2] is not None, place[v2][2] is not None
        pos2 = b2 - b1 if p1 and p2 else b2 - a1 if p2 else b1 - a2 if p1 else 0
        return [v1, v2, v1, v2, a2 - a1 + shift, pos2, fwd[v1], fwd[v2], ord("1")]

    rows, cliques, want = [], [], []
    filler = []  # vertices no clique names: the targets of the long lists' other records

    def clique(size, kinds, long_list=0, tie_step=None):
        a0 = int(rng.integers(200, template_len - 1200))
        vs = []
        for k in range(size):
            paired = {"s": False, "p": True, "m": bool(rng.random() < 0.5)}[kinds]
            if kinds == "m" and k == 0:
                paired = False
            # placements within 60 bases of one another: every pair overlaps; tie_step: equal lengths on a coarse grid, so that endpos ties
            a = a0 + (int(rng.integers(0, 4)) * tie_step if tie_step else int(rng.integers(0, 60)))
            vs.append(vertex(a, paired, l1=100 if tie_step else None))
        single = [v for v in vs if place[v][2] is None]
        base = single[0] if single else vs[0]
        groups = []  # the base's records per member
        for v in vs:
            if v == base:
                continue
            r = rng.random()
            if r < 0.55:
                groups.append([record(base, v)])
            elif r < 0.75:  # repeated: the first in list order wins
                groups.append([record(base, v), record(base, v, shift=3)])
            else:           # only in the member's list
                rows.append(record(v, base))
        n_own = sum(len(g) for g in groups)
        groups += [[record(base, int(t))] for t in rng.choice(filler, max(long_list - n_own, 0), replace=False)] if long_list else []
        for k in rng.permutation(len(groups)):  # not in target order
            rows.extend(groups[k])
        cliques.append([int(v) for v in rng.permutation(vs)])
        want.append(SR.SR_EDGE_OK)
        return vs

    for _ in range(220):
        filler.append(vertex(int(rng.integers(0, template_len - 400)), bool(rng.random() < 0.5)))
    for size, reps in ((2, 52), (3, 52), (12, 3), (13, 8), (16, 6), (17, 18), (40, 2)):
        for rep in range(reps):
            clique(size, "spm"[rep % 3], tie_step=20 if size >= 17 or (size > 12 and rep % 2) else None)
    for size in (63, 64, 65):
        clique(size, "s", tie_step=20)
    for n_list in (63, 64, 65, 200):
        clique(5, "m", long_list=n_list)
    # one clique per failing status
    ok = clique(4, "s")
    want.pop(), cliques.pop()
    far = [vertex(100, False), vertex(5000, False)]
    V = len(fwd) + 1  # the last vertex reads a read beyond the store
    bad = [([ok[0]], SR.SR_CLIQUE_TOO_SMALL), ([], SR.SR_CLIQUE_TOO_SMALL), ([ok[0], ok[1], ok[0]], SR.SR_CLIQUE_REPEATED_VERTEX),
           ([ok[0], ok[0]], SR.SR_EDGE_BAD_VERTEX), ([ok[0], ok[1], V + 5], SR.SR_EDGE_BAD_VERTEX), ([ok[0], V - 1, ok[1]], SR.SR_EDGE_BAD_VERTEX),
           ([far[0], far[1], ok[0]], SR.SR_EDGE_NO_EDGE), (ok, SR.SR_EDGE_OK)]
    for q, st in bad:
        cliques.append([int(v) for v in q])
        want.append(st)
    off = np.zeros(len(seq_len) + 1, np.uint64)
    off[1:] = np.cumsum(seq_len)
    n_reads = len(fwd)
    reads = ReadSet(np.concatenate(bases), np.concatenate(qual_parts), off, np.asarray(first, np.uint32), np.arange(n_reads, dtype=np.uint64))
    vertex_read = np.concatenate([np.arange(n_reads, dtype=np.uint32), [np.uint32(n_reads + 7)]]).astype(np.uint32)
    vertex_fwd = np.concatenate([np.asarray(fwd, np.uint8), [np.uint8(1)]]).astype(np.uint8)
    return dict(reads=reads, V=V, rows=rows, vertex_read=vertex_read, vertex_fwd=vertex_fwd, cliques=cliques, want_status=np.asarray(want, np.uint32), m=m)
