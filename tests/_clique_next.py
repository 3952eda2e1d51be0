"""Shared by tests/test_clique_next_host.py and tests/test_gpu_clique_next.py: hand-made inputs of hc_sr_clique_next (a store, consensus bytes
and a "clique merge result" written by hand, so that no graph is needed), a Python restatement of the reference lines the call stands for
(src/SRBuilder.cpp:981-1001, :1122-1222, with :911-935 in the call's documented tie order) composed over the existing mirrors of
merge_self_overlap and of the next store, and the comparison of two results array by array.  No reference code runs: the names say
"restatement"."""
import random
from dataclasses import dataclass

import numpy as np

from haploconduct_amd import clique_next as CN
from haploconduct_amd import consensus as SR
from haploconduct_amd import host as H
from haploconduct_amd import merge_next as MN
from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE
from haploconduct_amd.readstore import ReadSet
from tests._merge_next import _n_rate_ok, as_lists


@dataclass
class Case:
    reads: ReadSet
    cons_seq: np.ndarray
    cons_qual: np.ndarray
    clique_off: np.ndarray
    clique_nodes: np.ndarray
    merged: SR.SrCliqueLayouts
    vertex_read: np.ndarray
    vertex_fwd: np.ndarray


def merged_of(clique_status, first_layout, layouts, member_vertex, member_used, subreads, lay_status, out_off, cons_seq, cons_qual):
    res = SR.SrResult(np.zeros(len(lay_status), np.int32), np.array(lay_status, np.uint32), np.array(out_off, np.uint64), cons_seq, cons_qual, 0, 0, 0.0, 0.0)
    mv = np.array(member_vertex, np.uint32).reshape(-1)
    members = np.zeros(mv.size, SR.SR_MEMBER_DTYPE)
    return SR.SrCliqueLayouts(np.array(clique_status, np.uint32), np.array(first_layout, np.uint64), np.array(layouts, SR.SR_LAYOUT_DTYPE).reshape(-1),
                              members, mv, np.array(member_used, np.uint8).reshape(-1), np.zeros(len(lay_status), np.uint8),
                              np.array(subreads, SR.SR_SUBREAD_DTYPE).reshape(-1), result=res)


def make_case(seed, n_vertices, sizes, overlap=False, all_paired=False, unsorted=True, force=None):
    """n_vertices reads (vertex v <-> read perm[v]) and one clique per entry of `sizes` over them, with every shape of super-read: none,
    single-end from one layout, paired from two, empty mates, mates full of N, mates that overlap themselves.  overlap: cliques share
    vertices.  force: the style of every clique (a number in [0, 1), see below) instead of a drawn one."""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(3000))

    def qual(n):
        return "".join(rng.choice("5?FI") for _ in range(n))

    def seq(n, n_rate=0.0):
        a = rng.randrange(0, len(genome) - n)
        return "".join("N" if rng.random() < n_rate else c for c in genome[a:a + n])

    kinds = [all_paired or rng.random() < 0.6 for _ in range(n_vertices)]  # True: a paired read
    singles, paired = [], []
    for v in range(n_vertices):
        style = rng.random()
        ln = rng.choice((4, 7, 8)) if style < 0.15 else rng.randrange(20, 61)  # short ones for keep_singletons = 8
        nr = 0.2 if 0.15 <= style < 0.3 else 0.0
        if kinds[v]:
            l2 = rng.randrange(1, 5) if ln < 10 else rng.randrange(20, 61)
            paired.append(((seq(ln, nr), qual(ln)), (seq(l2, nr), qual(l2))))
        else:
            singles.append((seq(ln, nr), qual(ln)))
    reads = ReadSet.from_lists(singles, paired)
    order = list(range(n_vertices))
    rng.shuffle(order)
    vertex_read = np.zeros(n_vertices, np.uint32)
    ns, npd = 0, 0
    for v in order:
        if kinds[v]:
            vertex_read[v] = len(singles) + npd
            npd += 1
        else:
            vertex_read[v] = ns
            ns += 1
    vertex_fwd = np.array([rng.random() < 0.6 for _ in range(n_vertices)], np.uint8)
    # the cliques
    pool = list(range(n_vertices))
    rng.shuffle(pool)
    at = 0
    cliques = []
    for size in sizes:
        if overlap or at + size > n_vertices:
            cliques.append(rng.sample(range(n_vertices), size))
        else:
            cliques.append(pool[at:at + size])
            at += size
        if not unsorted:
            cliques[-1].sort()
    cs, cq, out_off = [], [], [0]
    clique_status, first_layout, layouts, member_vertex, member_used, subreads, lay_status = [], [0], [], [], [], [], []

    def layout(vs, size):
        layouts.append((len(member_vertex), len(vs), 100))
        member_vertex.extend(vs)
        # what filter_subreads would have left of a clique larger than 3 * min_clique_size: some members not handed to consensus
        member_used.extend([1 if size <= 6 or k % 3 else 0 for k in range(len(vs))])

    def emit(s, q, status=0):
        cs.append(s)
        cq.append(q)
        out_off.append(out_off[-1] + len(s))
        lay_status.append(status)

    for clique in cliques:
        ids = sorted(clique)
        style = rng.random() if force is None else force
        if style < 0.12 or len(ids) < 2:  # no super-read
            clique_status.append(rng.randrange(1, 8) if len(ids) >= 2 else 6)
            first_layout.append(first_layout[-1])
            subreads += [(-1, -1, -1, -1)] * len(ids)
            continue
        clique_status.append(0)
        if all(kinds[x] for x in ids):
            l, r = ids[:], ids[:]
            rng.shuffle(l)
            rng.shuffle(r)
            layout(l, len(ids))
            layout(r, len(ids))
            subreads += [(rng.choice((0, 0, 5, 20)), rng.randrange(3), rng.choice((0, 0, 5, 20)), rng.randrange(3)) for _ in ids]
            if style < 0.2:  # an empty mate
                emit(seq(30), qual(30))
                emit("", "")
            elif style < 0.3:  # too many N
                emit(seq(30, 0.3), qual(30))
                emit(seq(30, 0.3), qual(30))
            elif style < 0.65:  # mate 2 starts p bases into mate 1
                l1, l2 = rng.randrange(30, 70), rng.randrange(30, 70)
                p = rng.randrange(1, l1 - 20)
                a = rng.randrange(0, 2000)
                emit(genome[a:a + l1], "I" * l1)
                emit(genome[a + p:a + p + l2], "I" * l2)
            elif style < 0.7:  # a layout that is not HC_SR_OK counts as an empty mate, whatever its bytes
                emit(seq(30), qual(30))
                emit(seq(30), qual(30), status=4)
            else:
                n1, n2 = rng.randrange(20, 50), rng.randrange(20, 50)
                emit(seq(n1), qual(n1))
                emit(seq(n2), qual(n2))
            first_layout.append(first_layout[-1] + 2)
        else:
            vs = []
            for x in rng.sample(ids, len(ids)):
                vs += [x, x] if kinds[x] else [x]
            rng.shuffle(vs)
            layout(vs, len(ids))
            first_layout.append(first_layout[-1] + 1)
            subreads += [(rng.randrange(30), rng.randrange(3), rng.randrange(30) if kinds[x] else -1, rng.randrange(3) if kinds[x] else -1) for x in ids]
            if style < 0.2:
                emit("", "")
            elif style < 0.3:
                emit(seq(40, 0.3), qual(40))
            else:
                n = rng.randrange(20, 80)
                emit(seq(n), qual(n))
    cons_seq = np.frombuffer("".join(cs).encode(), np.uint8)
    cons_qual = np.frombuffer("".join(cq).encode(), np.uint8)
    merged = merged_of(clique_status, first_layout, layouts if layouts else np.zeros(0, SR.SR_LAYOUT_DTYPE), member_vertex, member_used,
                       subreads if subreads else np.zeros(0, SR.SR_SUBREAD_DTYPE), lay_status, out_off, cons_seq, cons_qual)
    clique_off = np.cumsum([0] + [len(c) for c in cliques]).astype(np.uint64)
    clique_nodes = np.array([x for c in cliques for x in c], np.uint32)
    return Case(reads, cons_seq, cons_qual, clique_off, clique_nodes, merged, vertex_read, vertex_fwd)


def clique(c, i):
    return [int(x) for x in c.clique_nodes[int(c.clique_off[i]):int(c.clique_off[i + 1])]]


def first_list(c, i):
    """sorted_vertices1 of clique i: member_vertex of its first layout"""
    L = c.merged.layouts[int(c.merged.first_layout[i])]
    a = int(L["first_member"])
    return [int(x) for x in c.merged.member_vertex[a:a + int(L["n_members"])]]


def merged_row_restatement(members, info):
    """src/SRBuilder.cpp:913-935 in hc_sr_clique_next's documented order: the entries by descending position of the vertex in the first
    layout's member list, index1 before index2, then a stable sort by index."""
    items = []
    for x in members[::-1]:
        items.append((info[x][0], x))
        if info[x][2] >= 0:
            items.append((info[x][2], x))
    items.sort(key=lambda t: t[0])
    return [x for _, x in items]


def restatement(c, keep_singletons=0, self_overlap=True, settings=None):
    """-> a dict of what hc_sr_clique_next returns, and the next store as [[(seq, qual), ...]]."""
    cs, cq = c.cons_seq.tobytes(), c.cons_qual.tobytes()
    m, n_cliques, nv = c.merged, len(c.clique_off) - 1, len(c.vertex_read)
    rs = c.reads
    sr = [None] * n_cliques  # the mates of clique i's super-read as constructSuperread returns it (:981)
    for i in range(n_cliques):
        vs = clique(c, i)
        if m.clique_status[i] != 0 or len(vs) < 2 or any(v >= nv for v in vs):
            continue
        l0, l1 = int(m.first_layout[i]), int(m.first_layout[i + 1])
        if l1 - l0 not in (1, 2):
            continue
        sr[i] = []
        for l in range(l0, l1):
            a, b = int(m.result.out_off[l]), int(m.result.out_off[l + 1])
            sr[i].append((cs[a:b], cq[a:b]) if m.result.status[l] == 0 else (b"", b""))
    # process_cliques, :982-1001
    cand = [i for i in range(n_cliques) if sr[i] is not None and len(sr[i]) == 2 and sr[i][0][0] and sr[i][1][0]] if self_overlap else []
    overlap_pos, score = np.full(n_cliques, -1, np.int32), np.zeros(n_cliques)
    if cand:
        seq, qual, sp = SR.pack_pairs([(sr[i][0][0], sr[i][0][1], sr[i][1][0], sr[i][1][1]) for i in cand])
        mm = H.sr_merge_self_overlaps(seq, qual, sp, settings=settings, count_first=True)
        for k, i in enumerate(cand):
            if mm.status[k] == SR.SR_SELF_MERGED:
                overlap_pos[i], score[i] = mm.overlap_pos[k], mm.score[k]
                sr[i] = [mm.merged(k)]
    kind = np.zeros(n_cliques, np.uint32)
    for i in range(n_cliques):
        if sr[i] is None:
            kind[i] = MN.MN_NONE
        elif any(len(x[0]) == 0 for x in sr[i]):  # :983, :999
            kind[i] = MN.MN_DROPPED_EMPTY
        elif not _n_rate_ok(b"".join(x[0] for x in sr[i])):  # :986, :999
            kind[i] = MN.MN_DROPPED_N_RATE
        else:
            kind[i] = MN.MN_SINGLE_SELF if overlap_pos[i] >= 0 else MN.MN_PAIRED if len(sr[i]) == 2 else MN.MN_SINGLE
    alive = kind >= MN.MN_SINGLE
    # :1122-1136
    visited = np.zeros(nv, np.uint8)
    for i in np.flatnonzero(alive):
        visited[first_list(c, i)] = 1
    # :1141-1142: the single-end super-reads take the first ids
    store, new_id = [], np.full(n_cliques, -1, np.int32)
    for i in range(n_cliques):
        if alive[i] and len(sr[i]) == 1:
            new_id[i] = len(store)
            store.append(sr[i])
    n_singles = len(store)
    # :1145-1222
    comp = {65: 84, 84: 65, 67: 71, 71: 67}
    state, node_id = np.zeros(nv, np.uint32), np.zeros(nv, np.uint64)
    for v in range(nv):
        if visited[v]:
            state[v] = MN.MN_V_MERGED
            continue
        r = int(c.vertex_read[v])
        q0 = int(rs.read_first_seq[r])
        mates = [rs.seq(q0 + k) for k in range(1 + rs.is_paired(r))]
        visited[v] = 1
        if sum(len(x[0]) for x in mates) < keep_singletons:  # :1149
            state[v] = MN.MN_V_SHORT
        elif not _n_rate_ok(b"".join(x[0] for x in mates)):  # :1155
            state[v] = MN.MN_V_N_RATE
        else:
            state[v] = MN.MN_V_TRIVIAL
            visited[v] = 0
            if not c.vertex_fwd[v]:  # :1191, :1204
                mates = [(bytes(comp.get(b, b) for b in s[::-1]), q[::-1]) for s, q in mates[::-1]]
            node_id[v] = len(store)  # :1219
            store.append(mates)
    n_trivials = len(store) - n_singles
    for i in range(n_cliques):  # :1233
        if alive[i] and len(sr[i]) == 2:
            new_id[i] = len(store)
            store.append(sr[i])
    # the tables
    nodes = np.zeros(nv, FNO_READ_DTYPE)
    for v in range(nv):
        r = int(c.vertex_read[v])
        q0 = int(rs.read_first_seq[r])
        nodes[v]["len1"] = len(rs.seq(q0)[0])
        nodes[v]["len2"] = len(rs.seq(q0 + 1)[0]) if rs.is_paired(r) else 0
        nodes[v]["paired"], nodes[v]["visited"], nodes[v]["orientation"], nodes[v]["id"] = rs.is_paired(r), visited[v], c.vertex_fwd[v], node_id[v]
    order = [i for i in range(n_cliques) if alive[i] and len(sr[i]) == 1] + [i for i in range(n_cliques) if alive[i] and len(sr[i]) == 2]
    srs, rows, subs = np.zeros(len(order), FNO_READ_DTYPE), [], []
    for k, i in enumerate(order):
        srs[k]["id"], srs[k]["len1"], srs[k]["paired"] = new_id[i], len(sr[i][0][0]), len(sr[i]) == 2
        srs[k]["len2"] = len(sr[i][1][0]) if len(sr[i]) == 2 else 0
        info = {}
        for j, x in enumerate(sorted(clique(c, i))):
            s = m.subreads[int(c.clique_off[i]) + j]
            i2 = int(s["index2"])
            if overlap_pos[i] >= 0 and i2 >= 0:
                i2 += int(overlap_pos[i])  # :918-922
            info[x] = (int(s["index1"]), int(s["startpos1"]), i2, int(s["startpos2"]))
            subs.append((x, info[x][0], info[x][2], info[x][1], info[x][3]))
        rows.append(merged_row_restatement(first_list(c, i), info) if overlap_pos[i] >= 0 else first_list(c, i))
    return dict(clique_kind=kind, clique_new_id=new_id, overlap_pos=overlap_pos, self_score=score, vertex_state=state, nodes=nodes, srs=srs,
                sr_clique=np.array(order, np.uint32), rows=rows, subreads=np.array(subs, FNO_SUBREAD_DTYPE) if subs else np.zeros(0, FNO_SUBREAD_DTYPE),
                subread_off=np.cumsum([0] + [int(c.clique_off[i + 1] - c.clique_off[i]) for i in order]), n_singles=n_singles, n_trivials=n_trivials,
                n_paired=len(store) - n_singles - n_trivials, new_read_count=len(store)), store


def check_against_restatement(got, want, store):
    for k in ("clique_kind", "clique_new_id", "overlap_pos", "self_score", "vertex_state", "sr_clique"):
        assert np.array_equal(getattr(got, k), want[k]), k
    for k in ("nodes", "srs", "subreads"):
        assert getattr(got, k).tobytes() == want[k].tobytes(), k
    assert [got.row(k).tolist() for k in range(len(got.srs))] == want["rows"]
    assert got.subread_off.tolist() == want["subread_off"].tolist()
    for k in ("n_singles", "n_trivials", "n_paired", "new_read_count"):
        assert getattr(got, k) == want[k], k
    assert got.empty == (len(store) == 0)
    if store and got.reads is not None:
        assert as_lists(got.reads) == store


def assert_same(a, b, what=""):
    """two CliqueNext results, every output array for equality"""
    for k in CN.ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k}"
    for k in ("n_singles", "n_trivials", "n_paired", "n_self_merged", "new_read_count", "empty"):
        assert getattr(a, k) == getattr(b, k), f"{what}: {k}"
    for k in ("n_kept", "n_dropped_empty", "n_dropped_n_rate", "n_dropped_short", "n_bad", "n_seq", "n_bytes"):
        assert a.counts[k] == b.counts[k], f"{what}: counts.{k}"


def call_host(c, **kw):
    return H.sr_clique_next(c.reads, c.cons_seq, c.cons_qual, c.clique_off, c.clique_nodes, c.merged, c.vertex_read, c.vertex_fwd, **kw)


KW_SETS = [dict(), dict(keep_singletons=8), dict(keep_singletons=9, self_overlap=False)]


def as_pairs_case(c):
    """a case whose cliques all have two vertices -> tests/_merge_next.Case for hc_sr_merge_next: members rebuilt so that a member's read names
    its vertex (hc_sr_merge_next finds the vertex of a member by its read)"""
    from tests import _merge_next as M

    m = c.merged
    members = np.zeros(m.member_vertex.size, SR.SR_MEMBER_DTYPE)
    members["read"] = c.vertex_read[m.member_vertex]
    edge = SR.SrEdgeLayouts(m.clique_status, m.first_layout, m.layouts, members, m.subreads.reshape(-1, 2), m.result)
    nv = len(c.vertex_read)
    return M.Case(c.reads, c.cons_seq, c.cons_qual, c.clique_nodes.reshape(-1, 2), edge, c.vertex_read, c.vertex_fwd, np.zeros(nv, np.uint8),
                  np.zeros(c.reads.n_reads, np.uint8))
