"""Shared by the tests of hc_fno3_from_originals and its mirror (include/hcsr.h): seeded dicts over reads of all three classes, the
reference's golden runs as dicts, and a restatement of the rule in plain Python — candidate pairs by shared original, SR1 by walk rank,
the shared original of smallest id, the ambiguity definition, deduceOverlap (reference src/FindNextOverlaps3.cpp:176-406) with its
float32 percentages — written from the header's text, not from the library's code."""
import json
import os
from collections import defaultdict

import numpy as np

from haploconduct_amd import fno as F
from haploconduct_amd import originals as OR
from haploconduct_amd.readstore import ReadSet
from tests import _fno as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fno", "fno3_run.json")
f32 = np.float32


class Stop(Exception):
    """The reference would assert / exit here (HC_ERR_FORMAT)."""


class TooMany(Exception):
    """More combinations than max_combos (HC_ERR_NOT_ON_DEVICE)."""


def i32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def ranks(counts3, walk_rank=None):
    ns, nt, npair = counts3
    if walk_rank is not None:
        return [int(x) for x in walk_rank]
    return [r if r < ns else r + npair if r < ns + nt else r - nt for r in range(ns + nt + npair)]


def _perc_max(ov, la, lb):
    a, b = f32(ov) / f32(la), f32(ov) / f32(lb)
    return int(np.floor(max(a, b) * f32(100.0)))


def _ratio100(a, b):
    return int(np.floor(f32(a) / f32(b) * f32(100.0)))


def deduce(A, B, oa, ob, no_inclusions):
    """A, B: (id, len1, len2, paired) of SR1 / SR2; oa, ob: (index1, index2) of the shared original in each.  -> the line or None."""
    (ida, A1, A2, ap), (idb, B1, B2, bp) = A, B
    (a_l, a_r), (b_l, b_r) = oa, ob
    a_first = a_l - b_l >= 0
    id1, id2 = (ida, idb) if a_first else (idb, ida)
    pos1, pos2, len2, perc2, ord_ = abs(a_l - b_l), 0, 0, 0, "-"
    if not ap and not bp:
        if pos1 > (A1 if a_first else B1):
            return None
        len1 = min(A1 - pos1, B1) if a_first else min(A1, B1 - pos1)
        perc1 = _perc_max(len1, A1, B1)
        t1 = t2 = "s"
    elif ap != bp:
        P1, P2, S = (A1, A2, B1) if ap else (B1, B2, A1)
        pair_first = ap == a_first
        len1 = P1 - pos1 if pair_first else min(P1, S - pos1)
        if len1 <= 0:
            return None
        t1, t2 = ("p", "s") if pair_first else ("s", "p")
        perc1 = _ratio100(len1, P1)
        pos2 = b_r - a_r if ap else a_r - b_r
        len2 = min(P2, S - pos2)
        if len2 <= 0 or pos2 < 0:
            return None
        perc2 = _ratio100(len2, P2)
    else:
        len1 = min(A1 - pos1, B1) if a_first else min(A1, B1 - pos1)
        back = a_r - b_r >= 0
        pos2 = abs(a_r - b_r)
        len2 = min(A2 - pos2, B2) if back else min(A2, B2 - pos2)
        if len1 <= 0 or len2 <= 0:
            return None
        perc1, perc2 = _perc_max(len1, A1, B1), _perc_max(len2, A2, B2)
        if not (0 <= perc1 <= 100 and 0 <= perc2 <= 100):
            raise Stop("the assert of :391")
        ord_ = "1" if a_first == back else "2"
        t1 = t2 = "p"
    if not (0 <= perc1 <= 100 and 0 <= perc2 <= 100) or len1 < 0 or len2 < 0:
        raise Stop("Overlap's constructor")
    perc = int(0.5 * (perc1 + perc2)) if perc2 > 0 else perc1
    if (no_inclusions and perc == 100) or len1 <= 0:
        return None
    return ("\t".join(str(x) for x in (id1, id2, pos1, pos2, ord_, "+", "+", perc1, perc2, len1, len2, t1, t2)) + "\n").encode()


def restate(off, entries, reads, counts3, original_readcount, walk_rank=None, max_combos=0, flags=0):
    """-> (text, counts without ms_device, candidates as a list of (a, b, original_id, flags))"""
    n = len(reads)
    rank = ranks(counts3, walk_rank)
    by_original = defaultdict(list)
    for r in range(n):
        for k in range(int(off[r]), int(off[r + 1])):
            by_original[int(entries[k]["id"])].append((rank[r], r, k))
    if len(by_original) > original_readcount:
        raise Stop("nodes_to_SR.at")
    n_combos = sum(len(m) * (len(m) - 1) // 2 for m in by_original.values())
    if n_combos > (max_combos or 2 ** 31 - 16):
        raise TooMany()
    shared = defaultdict(list)  # (rank of SR1, rank of SR2) -> its shared originals, ascending id
    for oid in sorted(by_original):
        m = sorted(by_original[oid])
        for i in range(len(m)):
            for j in range(i + 1, len(m)):
                shared[(m[i][0], m[j][0])].append((oid, m[i], m[j]))
    text, table, n_lines, n_amb = [], [], 0, 0
    for key in sorted(shared):
        oid, (_, a, ka), (_, b, kb) = shared[key][0]
        either = bool(reads[a]["paired"]) or bool(reads[b]["paired"])
        idx2 = lambda k: int(entries[k]["index2"]) if entries[k]["paired"] else 0
        diffs = {(i32(int(entries[x[2]]["index1"]) - int(entries[y[2]]["index1"])), i32(idx2(x[2]) - idx2(y[2])) if either else 0) for _, x, y in shared[key]}
        fl = OR.CAND_AMBIGUOUS if len(diffs) > 1 else 0
        n_amb += len(diffs) > 1
        fact = lambda r: (int(reads[r]["id"]), int(reads[r]["len1"]), int(reads[r]["len2"]) if reads[r]["paired"] else 0, bool(reads[r]["paired"]))
        line = deduce(fact(a), fact(b), (int(entries[ka]["index1"]), idx2(ka)), (int(entries[kb]["index1"]), idx2(kb)), bool(flags & F.NO_INCLUSIONS))
        if line is not None:
            text.append(line)
            fl |= OR.CAND_LINE
            n_lines += 1
        table.append((a, b, oid, fl))
    text = b"".join(text)
    return text, dict(n_lines=n_lines, n_bytes=len(text), candidates=len(table), n_combos=n_combos, n_ambiguous=n_amb, n_originals=len(by_original)), table


def same(got, want, what=""):
    """got: an originals.Fno3Resident; want: another one, or restate()'s triple."""
    if not isinstance(want, tuple):
        want = (want.text, {k: v for k, v in want.counts.items() if k != "ms_device"}, [tuple(int(x) for x in c) for c in want.candidates])
    text, counts, table = want
    assert {k: v for k, v in got.counts.items() if k != "ms_device"} == counts, what + ": counters"
    assert [tuple(int(x) for x in c) for c in got.candidates] == [tuple(c) for c in table], what + ": candidate table"
    assert got.text == text, what + ": text"


# ---- dicts ---------------------------------------------------------------------------------------------------------------------------
def to_csr(maps):
    """maps: per read a list of (id, index1, index2, len1, len2, paired) -> (off, entries), ascending id inside a read"""
    off = np.zeros(len(maps) + 1, np.uint64)
    rows = []
    for r, m in enumerate(maps):
        m = sorted(m)
        assert len({e[0] for e in m}) == len(m)
        off[r + 1] = off[r] + len(m)
        rows += [(e[0], e[1], e[2] if e[5] else 0, e[3], e[4] if e[5] else 0, e[5], 1, (0, 0)) for e in m]
    return off, np.array(rows, OR.ORIGINAL_DTYPE) if rows else np.zeros(0, OR.ORIGINAL_DTYPE)


def make_reads(lens, ids=None):
    """lens: per read (len1, len2, paired) -> FNO_READ_DTYPE, id = index unless given"""
    reads = np.zeros(len(lens), F.FNO_READ_DTYPE)
    for r, (l1, l2, p) in enumerate(lens):
        reads[r] = T.make_read(r if ids is None else int(ids[r]), l1, l2, int(p))
    return reads


def window_scenario(seed, counts3, n_originals, share=(1, 2, 3, 5), perturb=0.0, paired_trivials=0.4, axis=3000, paired_originals=True):
    """Every read is a window on one coordinate axis and every original a place on it: index1 = start(original) - start(read), and for a
    paired original index2 = start of its /2 - start of the read's /2 (of the read itself where it is single-end) — so every shared
    original of a pair tells the same (d_l, d_r); the originals are all paired or all single-end (index2 of a single-end original is 0
    whatever the read, so a mix would disagree in d_r).  perturb: the share of entries whose index1 is then moved, which makes pairs ambiguous.
    Ids run singles, trivials, pairs.  -> (off, entries, reads)"""
    rng = np.random.default_rng(seed)
    ns, nt, npair = counts3
    n = ns + nt + npair
    paired = np.array([False] * ns + [bool(rng.random() < paired_trivials) for _ in range(nt)] + [True] * npair)
    start1 = rng.integers(0, axis, n)
    len1, len2 = rng.integers(80, 500, n), rng.integers(80, 500, n)
    start2 = np.where(paired, start1 + len1 + rng.integers(0, 200, n), start1)
    maps = [[] for _ in range(n)]
    oids = rng.choice(np.arange(0, 20 * n_originals + 5), size=n_originals, replace=False)
    for oid in oids:
        s1, l1, l2, p = int(rng.integers(0, axis)), int(rng.integers(30, 150)), int(rng.integers(30, 150)), bool(paired_originals)
        s2 = s1 + l1 + int(rng.integers(0, 150))
        near = np.argsort(np.abs(start1 - s1) + rng.integers(0, 150, n))
        for r in near[:min(n, int(rng.choice(share)))]:
            i1 = s1 - int(start1[r])
            if perturb and rng.random() < perturb:
                i1 += int(rng.integers(1, 40))
            maps[int(r)].append((int(oid), i1, s2 - int(start2[r]), l1, l2, int(p)))
    off, entries = to_csr(maps)
    return off, entries, make_reads(list(zip(len1, np.where(paired, len2, 0), paired)))


def fno3_input(off, entries, reads, counts3, original_readcount, flags=0, seed=0):
    """The same data as an hc_fno3_input: the reads in walk order (singles, pairs, trivials), each one's originals shuffled."""
    rng = np.random.default_rng(seed)
    ns, nt, npair = counts3
    order = list(range(ns)) + list(range(ns + nt, ns + nt + npair)) + list(range(ns, ns + nt))
    originals = []
    for r in order:
        e = entries[int(off[r]):int(off[r + 1])]
        o = np.zeros(len(e), F.FNO_ORIGINAL_DTYPE)
        o["original_id"], o["index1"], o["index2"] = e["id"], e["index1"], np.where(e["paired"] != 0, e["index2"], 0)
        originals.append(o[rng.permutation(len(o))])
    return F.Fno3Input(reads[order], ns, npair, nt, originals, new_read_count=int(reads["id"].max()) + 1, original_readcount=original_readcount, flags=flags)


def golden_cases():
    """The reference's eight whole runs as (case, off, entries, reads in the golden order with the file's ids, counts3 for that order)."""
    out = []
    for c in json.load(open(GOLD))["cases"]:
        n_single, n_paired, n_trivial = c["counts"]
        srs, oo = c["srs"], c["orig_off"]
        maps = []
        for i in range(len(srs)):
            maps.append([(int(o[0]), int(o[1]), int(o[2]), 1, 1, 1) for o in c["originals_in_iteration_order"][oo[i]:oo[i + 1]]])
        off, entries = to_csr(maps)
        reads = make_reads([(s[1], s[2], s[3]) for s in srs], ids=[s[0] for s in srs])
        out.append((c, off, entries, reads, (n_single, n_trivial, n_paired)))
    return out


def lines_by_pair(text):
    d = {}
    for l in text.split(b"\n")[:-1]:
        a, b = l.split(b"\t")[:2]
        key = frozenset((int(a), int(b)))
        assert key not in d, "a pair wrote two lines"
        d[key] = l + b"\n"
    return d


def read_set(reads, seed=0):
    """A store of random bases with the reads' lengths and types, read r at index r (single-end and paired reads in any order)."""
    rng = np.random.default_rng(seed)
    lens, first = [], [0]
    for r in reads:
        lens += [int(r["len1"]), int(r["len2"])] if r["paired"] else [int(r["len1"])]
        first.append(len(lens))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total)]
    return ReadSet(bases, np.full(total, ord("I"), np.uint8), off, np.array(first, np.uint32), np.arange(len(reads), dtype=np.uint64))


def reads_of(rs):
    """FNO_READ_DTYPE per read of a ReadSet, id = index: what the device reads of its store's descriptors."""
    lens, first = np.diff(rs.seq_off.astype(np.int64)), rs.read_first_seq
    return make_reads([(lens[first[r]], lens[first[r] + 1] if rs.is_paired(r) else 0, rs.is_paired(r)) for r in range(rs.n_reads)])
