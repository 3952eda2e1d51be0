"""Shared by tests/test_merge_next_host.py and tests/test_gpu_merge_next.py: hand-made inputs of hc_sr_merge_next (a store, consensus bytes
and an "edge merge result" written by hand, so that no graph is needed), a Python restatement of the reference lines the call stands for
(src/SRBuilder.cpp:981-1001, :1260-1380) composed over the existing mirrors of merge_self_overlap and of the next store, and the comparison of
two results array by array.  No reference code runs: the names say "restatement"."""
import random
from dataclasses import dataclass

import numpy as np

from haploconduct_amd import consensus as SR
from haploconduct_amd import host as H
from haploconduct_amd import merge_next as MN
from haploconduct_amd import next_reads as NR
from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE
from haploconduct_amd.readstore import ReadSet


@dataclass
class Case:
    reads: ReadSet
    cons_seq: np.ndarray
    cons_qual: np.ndarray
    pairs: np.ndarray
    edge: SR.SrEdgeLayouts
    vertex_read: np.ndarray
    vertex_fwd: np.ndarray
    inclusions: np.ndarray
    tip_reads: np.ndarray


def edge_of(pair_status, first_layout, layouts, members, subreads, lay_status, out_off, cons_seq, cons_qual):
    res = SR.SrResult(np.zeros(len(lay_status), np.int32), np.array(lay_status, np.uint32), np.array(out_off, np.uint64), cons_seq, cons_qual, 0, 0, 0.0, 0.0)
    return SR.SrEdgeLayouts(np.array(pair_status, np.uint32), np.array(first_layout, np.uint64), np.array(layouts, SR.SR_LAYOUT_DTYPE).reshape(-1),
                            np.array(members, SR.SR_MEMBER_DTYPE).reshape(-1), np.array(subreads, SR.SR_SUBREAD_DTYPE).reshape(-1, 2), res)


def empty_edge():
    """the result of an edge merge of no pairs"""
    e = np.zeros(0, np.uint8)
    return edge_of([], [0], np.zeros(0, SR.SR_LAYOUT_DTYPE), np.zeros(0, SR.SR_MEMBER_DTYPE), np.zeros((0, 2), SR.SR_SUBREAD_DTYPE), [], [0], e, e)


def make_case(seed, n_vertices, n_pairs, reuse_vertex=False, all_paired=False):
    """n_vertices reads (vertex v <-> read perm[v]), n_pairs pairs over them with every shape of super-read: no super-read, single-end from one
    layout, paired from two, empty mates, mates full of N, mates that overlap themselves.  reuse_vertex: two pairs name one vertex."""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(3000))

    def qual(n):
        return "".join(rng.choice("5?FI") for _ in range(n))

    def seq(n, n_rate=0.0):
        a = rng.randrange(0, len(genome) - n)
        return "".join("N" if rng.random() < n_rate else c for c in genome[a:a + n])

    kinds = [all_paired or rng.random() < 0.5 for _ in range(n_vertices)]  # True: a paired read
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
    # reads are stored singles first: vertex v names the next single / paired read, in a shuffled vertex order
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
    inclusions = np.array([rng.random() < 0.2 for _ in range(n_vertices)], np.uint8)
    tip_reads = np.array([rng.random() < 0.2 for _ in range(n_vertices)], np.uint8)
    # the pairs
    pool = list(range(n_vertices))
    rng.shuffle(pool)
    pairs = []
    for i in range(n_pairs):
        if n_vertices < 2:
            pairs.append((0, 0))
        elif 2 * i + 1 < len(pool) and not (reuse_vertex and i % 3 == 2):
            pairs.append((pool[2 * i], pool[2 * i + 1]))
        else:
            v = pairs[rng.randrange(len(pairs))][0] if pairs else pool[0]
            w = rng.choice([x for x in range(n_vertices) if x != v])
            pairs.append((v, w))
    cs, cq, out_off = [], [], [0]
    pair_status, first_layout, layouts, members, subreads, lay_status = [], [0], [], [], [], []

    def layout(vs):
        layouts.append((len(members), len(vs), 100))
        for k, x in enumerate(vs):
            members.append((int(vertex_read[x]), 3 * k, 0, 0, (0, 0)))

    def emit(s, q, status=0):
        cs.append(s)
        cq.append(q)
        out_off.append(out_off[-1] + len(s))
        lay_status.append(status)

    for i, (v, w) in enumerate(pairs):
        lo, hi = min(v, w), max(v, w)
        style = rng.random()
        if style < 0.12:  # no super-read
            pair_status.append(rng.randrange(1, 6))
            first_layout.append(first_layout[-1])
            subreads.append([(-1, -1, -1, -1)] * 2)
            continue
        pair_status.append(0)
        both_paired = kinds[lo] and kinds[hi]
        if both_paired:
            first, second = (lo, hi) if rng.random() < 0.5 else (hi, lo)
            layout([first, second])
            layout([second, first] if rng.random() < 0.5 else [first, second])
            subreads.append([(rng.choice((0, 0, 5, 20)), rng.randrange(3), rng.choice((0, 0, 5, 20)), rng.randrange(3)) for _ in range(2)])
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
        else:
            vs = []
            for x in ((lo, hi) if rng.random() < 0.5 else (hi, lo)):
                vs += [x, x] if kinds[x] else [x]
            layout(vs)
            first_layout.append(first_layout[-1] + 1)
            subreads.append([(rng.randrange(30), rng.randrange(3), rng.randrange(30) if kinds[x] else -1, rng.randrange(3) if kinds[x] else -1)
                             for x in (lo, hi)])
            if style < 0.2:
                emit("", "")
            elif style < 0.3:
                emit(seq(40, 0.3), qual(40))
            else:
                n = rng.randrange(20, 80)
                emit(seq(n), qual(n))
            continue
        first_layout.append(first_layout[-1] + 2)
    cons_seq = np.frombuffer("".join(cs).encode(), np.uint8)
    cons_qual = np.frombuffer("".join(cq).encode(), np.uint8)
    edge = edge_of(pair_status, first_layout, layouts, members, subreads if subreads else np.zeros((0, 2), SR.SR_SUBREAD_DTYPE), lay_status, out_off,
                   cons_seq, cons_qual)
    return Case(reads, cons_seq, cons_qual, np.array(pairs, np.uint32).reshape(-1, 2), edge, vertex_read, vertex_fwd, inclusions, tip_reads)


def _n_rate_ok(seq):  # Read::test_N_rate, src/Read.h:214-234
    return float(seq.count(b"N")) < 0.05 * float(len(seq))


def merged_clique_restatement(first, second, info):
    """src/SRBuilder.cpp:913-935 for two keys: the map iterates `second` before `first` (the reverse of the insertion order of :571, as
    tests/golden/merge_next.json shows), each key gives (index1) and, where index2 >= 0, (index2); std::sort on four elements is stable."""
    items = []
    for key in (second, first):
        items.append((info[key][0], key))
        if info[key][2] >= 0:
            items.append((info[key][2], key))
    items.sort(key=lambda t: t[0])
    return [k for _, k in items]


def restatement(c, keep_singletons=0, ignore_inclusions=False, store_tips_separately=False, self_overlap=True, settings=None, use_inclusions=True,
                use_tips=True):
    """-> a dict of what hc_sr_merge_next returns, and the next store as [[(seq, qual), ...]]."""
    cs, cq = c.cons_seq.tobytes(), c.cons_qual.tobytes()
    e, n_pairs, nv = c.edge, len(c.pairs), len(c.vertex_read)
    rs = c.reads
    sr = [None] * n_pairs  # the mates of pair i's super-read as constructSuperread returns it (:981)
    for i in range(n_pairs):
        v, w = (int(x) for x in c.pairs[i])
        if e.pair_status[i] != 0 or v >= nv or w >= nv or v == w:
            continue
        l0, l1 = int(e.first_layout[i]), int(e.first_layout[i + 1])
        if l1 - l0 not in (1, 2):
            continue
        sr[i] = []
        for l in range(l0, l1):
            a, b = int(e.result.out_off[l]), int(e.result.out_off[l + 1])
            sr[i].append((cs[a:b], cq[a:b]) if e.result.status[l] == 0 else (b"", b""))
    # process_cliques, :982-1001
    cand = [i for i in range(n_pairs) if sr[i] is not None and len(sr[i]) == 2 and sr[i][0][0] and sr[i][1][0]] if self_overlap else []
    overlap_pos, score = np.full(n_pairs, -1, np.int32), np.zeros(n_pairs)
    if cand:
        seq, qual, sp = SR.pack_pairs([(sr[i][0][0], sr[i][0][1], sr[i][1][0], sr[i][1][1]) for i in cand])
        m = H.sr_merge_self_overlaps(seq, qual, sp, settings=settings, count_first=True)
        for k, i in enumerate(cand):
            if m.status[k] == SR.SR_SELF_MERGED:
                overlap_pos[i], score[i] = m.overlap_pos[k], m.score[k]
                sr[i] = [m.merged(k)]
    kind = np.zeros(n_pairs, np.uint32)
    for i in range(n_pairs):
        if sr[i] is None:
            kind[i] = MN.MN_NONE
        elif any(len(m[0]) == 0 for m in sr[i]):  # :983, :999
            kind[i] = MN.MN_DROPPED_EMPTY
        elif not _n_rate_ok(b"".join(m[0] for m in sr[i])):  # :986, :999
            kind[i] = MN.MN_DROPPED_N_RATE
        else:
            kind[i] = MN.MN_SINGLE_SELF if overlap_pos[i] >= 0 else MN.MN_PAIRED if len(sr[i]) == 2 else MN.MN_SINGLE
    alive = kind >= MN.MN_SINGLE
    # :1260-1277
    visited = np.zeros(nv, np.uint8)
    for i in np.flatnonzero(alive):
        visited[c.pairs[i]] = 1
    # :1279-1280: the single-end super-reads take the first ids
    store, new_id = [], np.full(n_pairs, -1, np.int32)
    for i in range(n_pairs):
        if alive[i] and len(sr[i]) == 1:
            new_id[i] = len(store)
            store.append(sr[i])
    n_singles = len(store)
    # :1282-1373
    comp = {65: 84, 84: 65, 67: 71, 71: 67}
    state, node_id, tips = np.zeros(nv, np.uint32), np.zeros(nv, np.uint64), []
    for v in range(nv):
        if visited[v]:
            state[v] = MN.MN_V_MERGED
            continue
        r = int(c.vertex_read[v])
        q0 = int(rs.read_first_seq[r])
        mates = [rs.seq(q0 + k) for k in range(1 + rs.is_paired(r))]
        visited[v] = 1
        if sum(len(m[0]) for m in mates) < keep_singletons:  # :1286
            state[v] = MN.MN_V_SHORT
        elif not _n_rate_ok(b"".join(m[0] for m in mates)):  # :1292
            state[v] = MN.MN_V_N_RATE
        elif ignore_inclusions and use_inclusions and c.inclusions[v]:  # :1298
            state[v] = MN.MN_V_INCLUSION
            tips.append(v)
        elif use_tips and c.tip_reads[r] and store_tips_separately:  # :1305
            state[v] = MN.MN_V_TIP
            tips.append(v)
        else:
            state[v] = MN.MN_V_TRIVIAL
            visited[v] = 0
            if not c.vertex_fwd[v]:  # :1342, :1355
                mates = [(bytes(comp.get(b, b) for b in s[::-1]), q[::-1]) for s, q in mates[::-1]]
            node_id[v] = len(store)  # :1370
            store.append(mates)
    n_trivials = len(store) - n_singles
    for i in range(n_pairs):  # :1378
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
    order = [i for i in range(n_pairs) if alive[i] and len(sr[i]) == 1] + [i for i in range(n_pairs) if alive[i] and len(sr[i]) == 2]
    srs, cliques, subs = np.zeros(len(order), FNO_READ_DTYPE), [], np.zeros(2 * len(order), FNO_SUBREAD_DTYPE)
    for k, i in enumerate(order):
        srs[k]["id"], srs[k]["len1"], srs[k]["paired"] = new_id[i], len(sr[i][0][0]), len(sr[i]) == 2
        srs[k]["len2"] = len(sr[i][1][0]) if len(sr[i]) == 2 else 0
        lo, hi = sorted(int(x) for x in c.pairs[i])
        info = {}
        for x, s in ((lo, e.subreads[i][0]), (hi, e.subreads[i][1])):
            i2 = int(s["index2"])
            if overlap_pos[i] >= 0 and i2 >= 0:
                i2 += int(overlap_pos[i])  # :918-922
            info[x] = (int(s["index1"]), int(s["startpos1"]), i2, int(s["startpos2"]))
            subs[2 * k + (x == hi)] = (x, info[x][0], info[x][2], info[x][1], info[x][3])
        L = e.layouts[int(e.first_layout[i])]
        mem = e.members[int(L["first_member"]):int(L["first_member"]) + int(L["n_members"])]
        who = [lo if int(c.vertex_read[lo]) == int(m["read"]) else hi for m in mem]
        cliques.append(merged_clique_restatement(who[0], hi if who[0] == lo else lo, info) if overlap_pos[i] >= 0 else who)
    return dict(pair_kind=kind, pair_new_id=new_id, overlap_pos=overlap_pos, self_score=score, vertex_state=state, nodes=nodes, srs=srs,
                sr_pair=np.array(order, np.uint32), cliques=cliques, subreads=subs, tips=np.array(tips, np.uint32), n_singles=n_singles,
                n_trivials=n_trivials, n_paired=len(store) - n_singles - n_trivials, new_read_count=len(store)), store


def as_lists(rs):
    return [[rs.seq(q) for q in range(int(rs.read_first_seq[r]), int(rs.read_first_seq[r + 1]))] for r in range(rs.n_reads)]


def check_against_restatement(got, want, store):
    for k in ("pair_kind", "pair_new_id", "overlap_pos", "self_score", "vertex_state", "sr_pair", "tips"):
        assert np.array_equal(getattr(got, k), want[k]), k
    for k in ("nodes", "srs", "subreads"):
        assert getattr(got, k).tobytes() == want[k].tobytes(), k
    assert [got.clique_nodes[int(got.clique_off[k]):int(got.clique_off[k + 1])].tolist() for k in range(len(got.srs))] == want["cliques"]
    assert got.subread_off.tolist() == [2 * k for k in range(len(got.srs) + 1)]
    for k in ("n_singles", "n_trivials", "n_paired", "new_read_count"):
        assert getattr(got, k) == want[k], k
    assert got.empty == (len(store) == 0)
    if store and got.reads is not None:
        assert as_lists(got.reads) == store


def assert_same(a, b, what=""):
    """two MergeNext results, every output array for equality"""
    for k in MN.ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k}"
    for k in ("n_singles", "n_trivials", "n_paired", "n_self_merged", "new_read_count", "empty"):
        assert getattr(a, k) == getattr(b, k), f"{what}: {k}"
    for k in ("n_kept", "n_dropped_empty", "n_dropped_n_rate", "n_dropped_short", "n_bad", "n_seq", "n_bytes"):
        assert a.counts[k] == b.counts[k], f"{what}: counts.{k}"


def call_host(c, **kw):
    return H.sr_merge_next(c.reads, c.cons_seq, c.cons_qual, c.pairs, c.edge, c.vertex_read, c.vertex_fwd, **kw)


KW_SETS = [dict(), dict(keep_singletons=8), dict(keep_singletons=8, ignore_inclusions=True, with_incl=True),
           dict(store_tips_separately=True, with_tips=True), dict(keep_singletons=9, ignore_inclusions=True, store_tips_separately=True, with_incl=True, with_tips=True),
           dict(self_overlap=False, ignore_inclusions=True, store_tips_separately=True)]


def split_kw(c, kw):
    """-> (the call's keywords, the restatement's) of one of KW_SETS: with_incl / with_tips pass the arrays, otherwise NULL"""
    kw = dict(kw)
    wi, wt = kw.pop("with_incl", False), kw.pop("with_tips", False)
    call = dict(kw, inclusions=c.inclusions if wi else None, tip_reads=c.tip_reads if wt else None)
    return call, dict(kw, use_inclusions=wi, use_tips=wt)
