"""hc_host_sr_clique_next and hc_host_sr_clique_select (include/hcsr.h) on the CPU.  Against tests/golden/clique_next.json (the reference's
calcSubreadInfo and merge_self_overlap on cliques of 3 - 40 vertices, and the gate of src/SRBuilder.cpp:1056-1084, run by
make_golden_clique_next.py): the subread map, overlap_pos and the merged read's sorted clique — as a sequence of index groups, inside a group
as a multiset of vertices (the reference's order there is the unordered_map's and an unstable sort's), and exactly in the call's documented
tie order.  Against a Python restatement of process_cliques' filters and of cliquesToSuperreads' loops (tests/_clique_next.py) on seeded
inputs.  And two-vertex cliques against hc_host_sr_merge_next."""
import json
import os

import numpy as np
import pytest

from tests import _clique_next as Q
from tests import _merge_next as M
from haploconduct_amd import host as H
from haploconduct_amd import merge_next as MN
from haploconduct_amd.readstore import ReadSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "clique_next.json")))
# (n_vertices, clique sizes)
SEEDED = [(1, []), (1, [1]), (5, [2, 3]), (63, [2, 3, 16, 17]), (64, [3] * 20), (65, [63]), (130, [64, 65]), (257, [200, 2, 5, 40]),
          (90, [2] * 10 + [3] * 10 + [5] * 8)]


def _golden_case():
    """every golden case as one clique of one call: the case's vertex ids renumbered in ascending order from `base` on"""
    g = GOLDEN
    cs, cq, out_off = [], [], [0]
    status, first_layout, layouts, member_vertex, subreads, lay_status, cliques, singles, backs = [], [0], [], [], [], [], [], [], []
    base = 0
    for i, c in enumerate(g["cases"]):
        m = g["mates"][c["mates"]]
        ids = sorted(c["v1"])
        assert sorted(c["v2"]) == ids and len(set(ids)) == len(ids)
        vertex = {x: base + k for k, x in enumerate(ids)}
        backs.append({v: x for x, v in vertex.items()})
        mine = [vertex[x] for x in c["v1"]]
        cliques.append(mine[::-1] if i % 2 else mine)  # (an unsorted clique)
        singles += [("ACGTACGTACGTACGTACGTA", "I" * 21)] * len(ids)  # read r = vertex r
        status.append(0)
        layouts.append((len(member_vertex), len(ids), 100))
        member_vertex += [vertex[x] for x in c["v1"]]
        layouts.append((len(member_vertex), len(ids), 100))
        member_vertex += [vertex[x] for x in c["v2"]]
        first_layout.append(first_layout[-1] + 2)
        rows = {r[0]: r[1:] for r in c["map"]}
        for x in ids:  # the map as calcSubreadInfo left it: the shift of :918-922 undone
            i1, s1, i2, s2 = rows[x]
            subreads.append((i1, s1, i2 - c["overlap_pos"] if c["merged"] and i2 >= 0 else i2, s2))
        for s, q in ((m["seq1"], m["qual1"]), (m["seq2"], m["qual2"])):
            cs.append(s)
            cq.append(q)
            out_off.append(out_off[-1] + len(s))
            lay_status.append(0)
        base += len(ids)
    cons_seq, cons_qual = np.frombuffer("".join(cs).encode(), np.uint8), np.frombuffer("".join(cq).encode(), np.uint8)
    merged = Q.merged_of(status, first_layout, layouts, member_vertex, np.ones(len(member_vertex), np.uint8), subreads, lay_status, out_off, cons_seq,
                         cons_qual)
    off = np.cumsum([0] + [len(x) for x in cliques]).astype(np.uint64)
    case = Q.Case(ReadSet.from_lists(singles), cons_seq, cons_qual, off, np.array([x for cl in cliques for x in cl], np.uint32), merged,
                  np.arange(base, dtype=np.uint32), np.ones(base, np.uint8))
    return g, case, backs


def _groups(vertices, index_of):
    """a row as a sequence of (index, sorted vertices of that index): `index_of` maps a vertex to its ascending list of indexes"""
    seen, out = {}, []
    for x in vertices:
        k = seen.get(x, 0)
        seen[x] = k + 1
        idx = index_of[x][k]
        if out and out[-1][0] == idx:
            out[-1][1].append(x)
        else:
            out.append((idx, [x]))
    return [(i, sorted(v)) for i, v in out]


def test_golden_subread_map_overlap_pos_and_sorted_clique_after_a_self_merge():
    g, case, backs = _golden_case()
    assert (g["min_score"], g["min_overlap"], g["min_qual"], g["mismatch"], g["min_read_len"]) == (0.99, 15, 0.99, 0.0, 0)
    got = Q.call_host(case)
    n_merged = n_ties = n_long = 0
    for i, c in enumerate(g["cases"]):
        back = backs[i]
        assert got.overlap_pos[i] == c["overlap_pos"], i
        assert got.clique_kind[i] == (MN.MN_SINGLE_SELF if c["merged"] else MN.MN_PAIRED), i
        k = int(np.flatnonzero(got.sr_clique == i)[0])
        sub = got.subreads[int(got.subread_off[k]):int(got.subread_off[k + 1])]
        assert [[back[int(s["node"])], int(s["index1"]), int(s["startpos1"]), int(s["index2"]), int(s["startpos2"])] for s in sub] == c["map"], i
        row = [back[int(x)] for x in got.row(k)]
        if not c["merged"]:
            assert row == c["v1"], i
            continue
        index_of = {r[0]: sorted([r[1]] + ([r[3]] if r[3] >= 0 else [])) for r in c["map"]}
        # a vertex with two entries meets its smaller index first in any index-sorted row: both rows resolve to the same (index, vertex) items
        assert _groups(row, index_of) == _groups(c["clique"], index_of), i
        idx = [j for j, grp in _groups(row, index_of) for _ in grp]
        assert idx == sorted(idx), i
        # the documented tie order
        info = {r[0]: (r[1], r[2], r[3], r[4]) for r in c["map"]}
        assert row == Q.merged_row_restatement(c["v1"], info), i
        n_merged += 1
        n_ties += len(set(idx)) < len(idx)
        n_long += len(row) > 16
    assert n_merged >= 60 and n_ties >= 20 and n_long >= 20, (n_merged, n_ties, n_long)
    assert got.n_self_merged == n_merged and got.n_trivials == 0 and not got.vertex_state.any()


def _csr(lines):
    """the vertices `iss >> node` reads from each line (:1061): integers up to the first token that is none"""
    cliques = []
    for line in lines:
        vs = []
        for tok in line.split():
            if not tok.isdigit():
                break
            vs.append(int(tok))
        cliques.append(vs)
    return np.cumsum([0] + [len(c) for c in cliques]).astype(np.uint64), np.array([x for c in cliques for x in c], np.uint32), cliques


def test_golden_clique_select():
    files = GOLDEN["select"]
    assert len(files) >= 40
    for f in files:
        off, nodes, cliques = _csr(f["lines"])
        for rmo, key in ((False, "plain"), (True, "remove_multi_occ")):
            got = H.sr_clique_select(off, nodes, f["n_vertices"], f["min_clique_size"], rmo)
            sel = [got.clique_nodes[int(got.clique_off[k]):int(got.clique_off[k + 1])].tolist() for k in range(len(got.index))]
            assert sel == f[key]["cliques"], (f, key)
            assert got.n_singletons == f[key]["n_singletons"], (f, key)
            assert np.all(np.diff(got.index.astype(np.int64)) > 0)
            for k, i in enumerate(got.index):  # a selected clique is its input clique without the vertices used before it
                assert [x for x in cliques[int(i)] if x in sel[k]] == sel[k] and (rmo or sel[k] == cliques[int(i)])
    # the file holds a clique that the filter reduces to a singleton ("2 3" after "0 1 2") and one that it leaves below minCliqueSize
    # ("1 2 3 4" after "0 1 2" with minCliqueSize 3: its vertices stay free for "3 4 5")
    a, b = files[-4], files[-3]
    assert a["lines"] == ["0 1 2", "2 3", "3 4 5"] and a["remove_multi_occ"] == dict(cliques=[[0, 1, 2], [3, 4, 5]], n_singletons=1)
    assert a["plain"]["n_singletons"] == 0
    assert b["min_clique_size"] == 3 and b["remove_multi_occ"] == dict(cliques=[[0, 1, 2], [3, 4, 5]], n_singletons=1)


def test_clique_select_refuses_a_vertex_outside_the_graph():
    with pytest.raises(Exception):
        H.sr_clique_select([0, 2], [0, 9], 9)


@pytest.mark.parametrize("nv,sizes", SEEDED)
@pytest.mark.parametrize("overlap", [False, True])
def test_restatement_seeded(nv, sizes, overlap):
    c = Q.make_case(2000 + nv * 7 + len(sizes), nv, sizes, overlap=overlap)
    for kw in Q.KW_SETS:
        got = Q.call_host(c, **kw)
        want, store = Q.restatement(c, **kw)
        Q.check_against_restatement(got, want, store)


def test_restatement_seeded_cases_take_every_branch():
    kinds, states, merged = set(), set(), 0
    for nv, sizes in SEEDED:
        got = Q.call_host(Q.make_case(2000 + nv * 7 + len(sizes), nv, sizes, overlap=True), keep_singletons=8)
        kinds |= set(got.clique_kind.tolist())
        states |= set(got.vertex_state.tolist())
        merged += got.n_self_merged
    assert kinds == set(range(6)) and states >= {MN.MN_V_MERGED, MN.MN_V_TRIVIAL, MN.MN_V_SHORT, MN.MN_V_N_RATE} and merged > 3


def test_a_self_merged_clique_of_many_vertices():
    c = Q.make_case(77, 80, [40, 33], all_paired=True, force=0.5)
    got = Q.call_host(c)
    assert got.n_self_merged == 2 and [len(got.row(k)) for k in range(2)] == [80, 66]
    want, store = Q.restatement(c)
    Q.check_against_restatement(got, want, store)


@pytest.mark.parametrize("seed,nv,n", [(1, 2, 1), (2, 64, 32), (3, 131, 65), (4, 40, 30)])
def test_two_vertex_cliques_equal_merge_next(seed, nv, n):
    c = Q.make_case(seed, nv, [2] * n, overlap=2 * n > nv)
    p = Q.as_pairs_case(c)
    for kw in Q.KW_SETS:
        a, b = Q.call_host(c, **kw), M.call_host(p, **kw)
        for ka, kb in (("clique_kind", "pair_kind"), ("clique_new_id", "pair_new_id"), ("sr_clique", "sr_pair")):
            assert np.array_equal(getattr(a, ka), getattr(b, kb)), ka
        for k in ("overlap_pos", "self_score", "vertex_state", "nodes", "srs", "clique_off", "clique_nodes", "subread_off", "subreads"):
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
        for k in ("n_singles", "n_trivials", "n_paired", "n_self_merged", "new_read_count", "empty", "counts"):
            assert getattr(a, k) == getattr(b, k), k
        if not a.empty:
            assert M.as_lists(a.reads) == M.as_lists(b.reads)


def _tweak(c, **kw):
    """a copy of the case with fields of its clique merge result replaced"""
    import copy

    c = copy.copy(c)
    c.merged = copy.copy(c.merged)
    for k, v in kw.items():
        setattr(c if hasattr(c, k) else c.merged, k, v)
    return c


def test_refusals_per_clique_and_for_the_call():
    c = Q.make_case(5, 30, [3, 4, 5], force=0.9)
    good = Q.call_host(c)
    assert (good.clique_kind >= MN.MN_SINGLE).all()
    nodes = c.clique_nodes.copy()
    nodes[4] = 30  # a vertex of clique 1 that is not the graph's
    got = Q.call_host(_tweak(c, clique_nodes=nodes))
    assert got.clique_kind.tolist()[1] == MN.MN_NONE and got.clique_kind[0] == good.clique_kind[0] and got.clique_kind[2] == good.clique_kind[2]
    assert all(got.vertex_state[v] != MN.MN_V_MERGED for v in Q.clique(c, 1))  # its vertices come back as trivials or are dropped as such
    mv = c.merged.member_vertex.copy()
    mv[int(c.merged.layouts[int(c.merged.first_layout[2])]["first_member"])] = 1000
    assert Q.call_host(_tweak(c, member_vertex=mv)).clique_kind.tolist()[2] == MN.MN_NONE
    fl = c.merged.first_layout.copy()
    fl[1] = fl[2]  # clique 0 takes clique 1's layouts too, clique 1 is left without
    kinds = Q.call_host(_tweak(c, first_layout=fl)).clique_kind.tolist()
    assert kinds[1] == MN.MN_NONE and (kinds[0] == MN.MN_NONE) == (int(fl[1]) > 2)
    lay = c.merged.layouts.copy()
    lay["n_members"][int(c.merged.first_layout[2])] = 10 ** 6  # a member range outside the array
    assert Q.call_host(_tweak(c, layouts=lay)).clique_kind.tolist()[2] == MN.MN_NONE
    oo = c.merged.result.out_off.copy()
    l0 = int(c.merged.first_layout[1])
    oo[l0 + 1] = oo[l0] - 1 if oo[l0] else 2 ** 40  # descending, or beyond a read's length
    import copy

    res = copy.copy(c.merged.result)
    res.out_off = oo
    assert Q.call_host(_tweak(c, result=res)).clique_kind.tolist()[1] == MN.MN_NONE
    # for the whole call
    with pytest.raises(Exception):
        Q.call_host(_tweak(c, clique_off=np.array([0, 7, 3, 12], np.uint64)))
    lay = c.merged.layouts.copy()
    a, b = int(c.merged.first_layout[0]), int(c.merged.first_layout[1])
    lay[[a, b]] = lay[[b, a]]  # the first layouts' member ranges no longer ascend
    with pytest.raises(Exception):
        Q.call_host(_tweak(c, layouts=lay))
