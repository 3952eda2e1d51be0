"""Shared by tests/test_originals_host.py and tests/test_gpu_originals.py: hand-made inputs of hc_sr_originals_next (a dict, and the tables a
merge call would have returned, written by hand so that no graph is needed), a plain-Python restatement of the reference lines the call
stands for (src/SRBuilder.cpp:750-806, :938-949, :1161-1216, :1449-1463; src/OverlapGraph.cpp:772-838) over dicts of Python integers, and
the conversions between a CSR dict and a list of maps.  No reference code runs: the names say "restatement"."""
import random

import numpy as np

from haploconduct_amd import merge_next as MN
from haploconduct_amd import originals as OR
from haploconduct_amd.consensus import SR_LAYOUT_DTYPE
from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE

I32 = (-(1 << 31), (1 << 31) - 1)


def to_csr(maps):
    """a list of {id: dict(index1, index2, len1, len2, paired, forward)} -> (off, entries), ascending id"""
    off, rows = [0], []
    for m in maps:
        for oid in sorted(m):
            e = m[oid]
            p = bool(e["paired"])
            rows.append((oid, e["index1"], e["index2"] if p else 0, e["len1"], e["len2"] if p else 0, p, bool(e["forward"]), (0, 0)))
        off.append(len(rows))
    return np.array(off, np.uint64), np.array(rows, OR.ORIGINAL_DTYPE) if rows else np.zeros(0, OR.ORIGINAL_DTYPE)


def to_maps(off, entries):
    out = []
    for r in range(len(off) - 1):
        m = {}
        for e in entries[int(off[r]):int(off[r + 1])]:
            m[int(e["id"])] = dict(index1=int(e["index1"]), index2=int(e["index2"]), len1=int(e["len1"]), len2=int(e["len2"]), paired=bool(e["paired"]),
                                   forward=bool(e["forward"]))
        out.append(m)
    return out


def first_it_restatement(nodes_len1, nodes_len2, paired):
    """OverlapGraph::buildOriginalsDict with first_it, src/OverlapGraph.cpp:772-797"""
    return [{r: dict(index1=0, index2=0, len1=int(nodes_len1[r]), len2=int(nodes_len2[r]) if paired[r] else 0, paired=bool(paired[r]), forward=True)}
            for r in range(len(paired))]


def next_restatement(maps, t):
    """-> (the new maps, a failed read's is None; the statuses).  maps: the dict of the store the merge call found; t: an originals.Tables."""
    n_new = int(t.new_read_count)
    new, bits = [dict() for _ in range(n_new)], [0] * n_new
    for k, c in enumerate(int(x) for x in t.sr_clique):
        nid = int(t.new_id[c])
        two = int(t.first_layout[c + 1]) - int(t.first_layout[c]) == 2
        len2 = int(t.layouts[int(t.first_layout[c]) + 1]["total_len"]) if two else 0  # sort_vertices(clique, 'r', ...), :693
        merged, op = t.kind[c] == MN.MN_SINGLE_SELF, int(t.overlap_pos[c])
        originals = new[nid]
        for j in range(int(t.subread_off[k]), int(t.subread_off[k + 1])):  # for (auto node_it : clique), :752
            row = t.subreads[j]
            v = int(row["node"])
            sub_id, node, forward = int(t.vertex_read[v]), t.nodes[v], bool(t.vertex_fwd[v])  # :753-755
            sub_index2 = int(row["index2"])
            if merged and sub_index2 >= 0:
                sub_index2 -= op  # the row as constructSuperread saw it: :918-922 not yet applied
            idx1 = int(row["index1"]) - int(row["startpos1"])  # :758
            idx2 = sub_index2 - int(row["startpos2"])          # :759
            seq1 = seq0 = int(node["len1"])
            seq2 = int(node["len2"])
            for oid, src in maps[sub_id].items():  # :760
                if oid in originals:
                    continue  # :762-764
                e = dict(src)
                e["forward"] = e["forward"] == forward  # :766
                if t.first_it:  # :767-772
                    e["index1"] = idx1
                    if e["paired"]:
                        e["index2"] = idx2
                elif forward:  # :773-783
                    e["index1"] += idx1
                    if e["paired"]:
                        e["index2"] += idx2 if sub_index2 >= 0 else idx1
                elif e["paired"]:
                    if node["paired"]:  # :786-794
                        e["index1"] = seq1 + idx1 - (e["len1"] + e["index1"])
                        if len2 > 0 or sub_index2 >= 0:
                            e["index2"] = seq2 + idx2 - (e["len2"] + e["index2"])
                        else:
                            e["index2"] = seq2 + idx1 - (e["len2"] + e["index2"])
                    else:  # :795-798
                        e["index1"] = seq0 + idx1 - (e["len1"] + e["index1"])
                        e["index2"] = seq0 + idx1 - (e["len2"] + e["index2"])
                elif node["paired"]:
                    bits[nid] |= 2  # get_seq(0) of a paired read, :801 -> the assert of Read.h:145-149
                else:
                    e["index1"] = seq0 + idx1 - (e["len1"] + e["index1"])  # :801
                originals[oid] = e  # :805
        if merged:  # :938-949
            for e in originals.values():
                if e["paired"]:
                    e["index2"] += op
    for v in range(len(t.vertex_read)):
        if t.vertex_state[v] != MN.MN_V_TRIVIAL:
            continue
        nid, node, src = int(t.nodes[v]["id"]), t.nodes[v], maps[int(t.vertex_read[v])]
        if not src:
            bits[nid] |= 1  # assert (subreads.size() > 0), :1178
        for oid, e in src.items():
            e = dict(e)
            if not t.vertex_fwd[v]:  # :1193-1199, :1206-1213
                e["forward"] = not e["forward"]
                if node["paired"]:
                    e["index1"] = int(node["len1"]) - (e["index1"] + e["len1"])
                    if e["paired"]:  # (the reference also writes index2 of a single-end original here: never printed, 0 in this project)
                        e["index2"] = int(node["len2"]) - (e["index2"] + e["len2"])
                else:
                    e["index1"] = int(node["len1"]) - (e["index1"] + e["len1"])
                    if e["paired"]:
                        e["index2"] = int(node["len1"]) - (e["index2"] + e["len2"])
            new[nid][oid] = e
    status = []
    for r in range(n_new):
        for e in new[r].values():
            if not I32[0] <= e["index1"] <= I32[1] or (e["paired"] and not I32[0] <= e["index2"] <= I32[1]):
                bits[r] |= 4
        status.append(OR.ORIG_EMPTY_SOURCE if bits[r] & 1 else OR.ORIG_SEQ0_OF_PAIRED if bits[r] & 2 else OR.ORIG_RANGE if bits[r] & 4 else OR.ORIG_OK)
        if status[r]:
            new[r] = None
    return new, np.array(status, np.uint32)


def text_restatement(maps):
    """the writers, src/SRBuilder.cpp:1449-1463, a line per read in id order, entries in ascending original id (this project's order)"""
    out = []
    for r, m in enumerate(maps):
        line = str(r)
        for oid in sorted(m or {}):
            e = m[oid]
            line += f"\t{oid}:{'+' if e['forward'] else '-'}:{e['index1']}"
            line += f",{e['index2']}:{e['len1']},{e['len2']}" if e["paired"] else f":{e['len1']}"
        out.append(line + "\n")
    return "".join(out).encode()


def make_case(seed, n_vertices, sizes, dict_sizes=(1, 2, 3), n_orig=None, first_it=False, seq0=False, wide=False, empty=0.0, share=False, short=0.1):
    """n_vertices vertices (vertex v <-> read perm[v]), a dict whose reads own dict_sizes-many originals out of a pool of n_orig ids (a small
    pool: members share originals, and the winner rule decides), and one super-read per entry of `sizes` over sorted vertex samples, of every
    kind; the vertices no super-read uses are trivials, a few of them too short.  seq0: single-end originals may sit in paired reads under
    reverse vertices (HC_SR_ORIG_SEQ0_OF_PAIRED where not first_it; "fwd": under forward vertices only); wide: indices near the int32 limits (HC_SR_ORIG_RANGE); empty: the share
    of reads with no original; share: every member of a super-read owns the same originals; short: the share of unused vertices that are no
    trivials.
    -> (maps, originals.Tables)"""
    rng = random.Random(seed)
    nv = n_vertices
    paired_read = [rng.random() < 0.5 for _ in range(nv)]
    perm = list(range(nv))
    rng.shuffle(perm)
    n_orig = n_orig or max(4, 2 * nv)
    maps = []
    for r in range(nv):
        m = {}
        k = 0 if rng.random() < empty else rng.choice(dict_sizes)
        for oid in rng.sample(range(n_orig), min(k, n_orig)):
            p = rng.random() < 0.5 if (seq0 or not paired_read[r]) else True
            big = wide and rng.random() < 0.2
            m[oid] = dict(index1=rng.choice((-2147483600, 2147483600, 123456789)) if big else rng.randrange(-40, 400),
                          index2=(rng.randrange(-40, 400) if p else 0), len1=rng.randrange(30, 251), len2=rng.randrange(30, 251) if p else 0, paired=p,
                          forward=rng.random() < 0.5)
        maps.append(m)
    nodes = np.zeros(nv, FNO_READ_DTYPE)
    vertex_read, vertex_fwd = np.zeros(nv, np.uint32), np.zeros(nv, np.uint8)
    for v in range(nv):
        r = perm[v]
        vertex_read[v] = r
        vertex_fwd[v] = rng.random() < 0.5
        nodes[v]["len1"], nodes[v]["len2"], nodes[v]["paired"] = rng.randrange(40, 300), rng.randrange(40, 300) if paired_read[r] else 0, paired_read[r]
        nodes[v]["orientation"] = vertex_fwd[v]
    kind, overlap_pos, first_layout, layouts, cliques = [], [], [0], [], []
    for size in sizes:
        vs = sorted(rng.sample(range(nv), size))
        if share:
            for v in vs[1:]:
                maps[perm[v]] = {oid: dict(e, index1=e["index1"] + 1) for oid, e in maps[perm[vs[0]]].items()}
        style = rng.random()
        all_paired = all(paired_read[perm[v]] for v in vs)
        if style < 0.15:
            k = rng.choice((MN.MN_NONE, MN.MN_DROPPED_EMPTY, MN.MN_DROPPED_N_RATE))
        elif all_paired:
            k = MN.MN_SINGLE_SELF if style < 0.5 else MN.MN_PAIRED
        else:
            k = MN.MN_SINGLE
        n_lay = 0 if k == MN.MN_NONE else 2 if all_paired else 1
        for l in range(n_lay):
            layouts.append((0, size, rng.choice((0, 180)) if l else 150))
        first_layout.append(first_layout[-1] + n_lay)
        kind.append(k)
        overlap_pos.append(rng.randrange(0, 120) if k == MN.MN_SINGLE_SELF else -1)
        cliques.append(vs)
    alive = [i for i, k in enumerate(kind) if k >= MN.MN_SINGLE]
    used = set(v for i in alive for v in cliques[i])
    new_id = [-1] * len(sizes)
    n = 0
    for i in alive:
        if kind[i] != MN.MN_PAIRED:
            new_id[i] = n
            n += 1
    state = np.zeros(nv, np.uint32)
    for v in range(nv):
        if v in used:
            state[v] = MN.MN_V_MERGED
            nodes[v]["visited"] = 1
        elif rng.random() < short:
            state[v] = MN.MN_V_SHORT
            nodes[v]["visited"] = 1
        else:
            state[v] = MN.MN_V_TRIVIAL
            nodes[v]["id"] = n
            n += 1
    for i in alive:
        if kind[i] == MN.MN_PAIRED:
            new_id[i] = n
            n += 1
    order = [i for i in alive if kind[i] != MN.MN_PAIRED] + [i for i in alive if kind[i] == MN.MN_PAIRED]
    subs, sub_off = [], [0]
    for i in order:
        for v in cliques[i]:
            has2 = paired_read[perm[v]] and rng.random() < 0.8
            i2 = rng.randrange(0, 300) if has2 else -1  # (-1: the dummy of a read with no second index)
            if kind[i] == MN.MN_SINGLE_SELF and i2 >= 0:
                i2 += overlap_pos[i]  # as the merge call returns it, :918-922
            subs.append((v, rng.randrange(0, 300), i2, rng.randrange(0, 4), rng.randrange(0, 4) if has2 else -1))
        sub_off.append(len(subs))
    if seq0 == "fwd":  # single-end originals in paired reads under forward vertices only: the combination :801 does not assert on
        for v in range(nv):
            if paired_read[perm[v]] and not vertex_fwd[v]:
                for e in maps[perm[v]].values():
                    if not e["paired"]:
                        e.update(paired=True, index2=rng.randrange(-40, 400), len2=rng.randrange(30, 251))
    t = OR.Tables(np.array(kind, np.uint32), np.array(new_id, np.int32), np.array(overlap_pos, np.int32), np.array(first_layout, np.uint64),
                  np.array(layouts, SR_LAYOUT_DTYPE) if layouts else np.zeros(0, SR_LAYOUT_DTYPE), np.array(order, np.uint32), np.array(sub_off, np.uint64),
                  np.array(subs, FNO_SUBREAD_DTYPE) if subs else np.zeros(0, FNO_SUBREAD_DTYPE), state, nodes, vertex_read, vertex_fwd, n, first_it)
    return maps, t


def assert_dict_equals_maps(off, entries, maps, what=""):
    want_off, want = to_csr([m if m is not None else {} for m in maps])  # (a failed read has no entries)
    assert off.tolist() == want_off.tolist(), f"{what}: offsets"
    assert entries.tobytes() == want.tobytes(), f"{what}: entries"
