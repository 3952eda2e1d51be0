"""Shared by the branch-evidence tests and tests/golden/make_golden_branch_evidence.py: a seeded maker of cases (a short genome with haplotype
variants, contigs and original reads cut from it, so that edges are real overlaps), hand-built cases from explicit tables, a Python
RESTATEMENT of reference src/BranchReduction.cpp:229-743 with the caller's loops (:60-80), and the comparison of a BranchEvidence with it.

The restatement is written from the cited lines, statement by statement, with Python strings and lists; it is not the reference (the
golden file is) but an independent second reading of it that runs on any case."""
from dataclasses import dataclass, field

import numpy as np

from haploconduct_amd import branch_evidence as BR
from haploconduct_amd.host import EDGE_DTYPE
from haploconduct_amd.originals import ORIGINAL_DTYPE
from haploconduct_amd.readstore import ReadSet

COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N"}


def rev_comp(s):
    return "".join(COMP[c] for c in reversed(s))


def i32(x):
    """an int cut to 32 bits, as an assignment to int does"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


@dataclass
class Case:
    """Everything one call reads.  Vertex v is read vertex_read[v]; the store holds single-end reads unless `paired` names reads that get a
    second sequence.  edges: (u, v, pos1) in adj_out order per u (any order of targets); adj_in order is in_order or ascending insertion."""
    name: str
    seqs: list                # per READ: the stored sequence
    vertex_read: list
    vertex_fwd: list
    edges: list               # (u, v, pos1), grouped by u in list order
    dicts: list               # per READ: [(id, index1, forward)] in ascending id
    originals: list           # sequences as stored
    se_count: int
    pe_count: int
    original_readcount: int
    min_overlap_len: int = 10
    edge_threshold: float = 0.97
    paired: dict = field(default_factory=dict)  # read -> second sequence
    in_lists: dict = None     # vertex -> sources in adj_in order (default: in order of the edges)

    @property
    def n_vertices(self):
        return len(self.vertex_read)

    def reads(self):
        singles = [(self.seqs[r], "I" * len(self.seqs[r])) for r in range(len(self.seqs))]
        # the store keeps the reads in index order: build the arrays directly so that a paired read may sit anywhere
        seqs, first = [], [0]
        for r, (s, _) in enumerate(singles):
            seqs.append(s)
            if r in self.paired:
                seqs.append(self.paired[r])
            first.append(len(seqs))
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        bases = np.frombuffer("".join(seqs).encode(), np.uint8) if seqs else np.zeros(0, np.uint8)
        return ReadSet(bases, np.full(bases.size, ord("I"), np.uint8), off, np.array(first, np.uint32), np.arange(len(singles), dtype=np.uint64))

    def graph(self):
        V = self.n_vertices
        by_u = [[] for _ in range(V)]
        for u, v, pos in self.edges:
            by_u[u].append((v, pos))
        recs, out_off = [], [0]
        for u in range(V):
            for v, pos in by_u[u]:
                recs.append((u, v, pos))
            out_off.append(len(recs))
        edges = np.zeros(len(recs), EDGE_DTYPE)
        for k, (u, v, pos) in enumerate(recs):
            e = edges[k]
            e["score"], e["mismatch_rate"], e["pos1"] = 0.99, 0.0, pos
            e["ori1"], e["ori2"], e["ord"] = self.vertex_fwd[u], self.vertex_fwd[v], ord("-")
            e["read1"], e["read2"], e["v1"], e["v2"] = self.vertex_read[u], self.vertex_read[v], u, v
            e["perc"], e["len0"], e["len1"] = 50, 20, 20
        ins = [[] for _ in range(V)]
        for u, v, _ in recs:
            ins[v].append(u)
        if self.in_lists:
            for v, l in self.in_lists.items():
                assert sorted(l) == sorted(ins[v])
                ins[v] = list(l)
        in_off = np.zeros(V + 1, np.uint64)
        in_off[1:] = np.cumsum([len(l) for l in ins])
        in_nodes = np.array([u for l in ins for u in l], np.uint32)
        return dict(edges=edges, out_off=np.array(out_off, np.uint64), in_nodes=in_nodes, in_off=in_off)

    def dict_arrays(self):
        off, rows = [0], []
        for d in self.dicts:
            assert [x[0] for x in d] == sorted(set(x[0] for x in d))
            rows += d
            off.append(len(rows))
        entries = np.zeros(len(rows), ORIGINAL_DTYPE)
        for k, (oid, index1, fwd) in enumerate(rows):
            ln = len(self.originals[oid]) if oid < len(self.originals) else 30
            entries[k] = (oid, index1, 0, ln, 0, 0, fwd, (0, 0))
        return np.array(off, np.uint64), entries

    def original_arrays(self):
        off = np.zeros(len(self.originals) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in self.originals])
        return np.frombuffer("".join(self.originals).encode(), np.uint8) if self.originals else np.zeros(0, np.uint8), off

    def settings(self):
        return BR.settings(self.se_count, self.pe_count, self.original_readcount, self.min_overlap_len, self.edge_threshold)

    def to_json(self):
        return dict(name=self.name, seqs=self.seqs, vertex_read=self.vertex_read, vertex_fwd=self.vertex_fwd, edges=[list(e) for e in self.edges],
                    dicts=[[list(x) for x in d] for d in self.dicts], originals=self.originals, se_count=self.se_count, pe_count=self.pe_count,
                    original_readcount=self.original_readcount, min_overlap_len=self.min_overlap_len, edge_threshold=self.edge_threshold,
                    in_lists={str(k): v for k, v in (self.in_lists or {}).items()})

    @classmethod
    def from_json(cls, j):
        return cls(j["name"], j["seqs"], j["vertex_read"], j["vertex_fwd"], [tuple(e) for e in j["edges"]], [[tuple(x) for x in d] for d in j["dicts"]],
                   j["originals"], j["se_count"], j["pe_count"], j["original_readcount"], j["min_overlap_len"], j["edge_threshold"],
                   in_lists={int(k): v for k, v in j["in_lists"].items()} or None)


def host_run(case, n_threads=1):
    from haploconduct_amd import host

    off, entries = case.dict_arrays()
    ob, oo = case.original_arrays()
    return host.br_evidence(case.graph(), case.reads(), off, entries, ob, oo, case.vertex_read, case.vertex_fwd, case.settings(), n_threads)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

class Failed(Exception):
    def __init__(self, status):
        self.status = status


def restate(case):
    """-> dict(branches=[dict(node, side, status, is_false, dist, final, diffs, n)], evidence={(u, v): [ids]}, missing=[dict])"""
    V = case.n_vertices
    g = case.graph()
    edges, out_off, in_off, in_nodes = g["edges"], g["out_off"], g["in_off"], g["in_nodes"]
    # sortAdjOut (:48): the tests' lists never repeat a target in a list of more than 16 entries, where std::sort is not stable
    adj_out = [sorted(range(int(out_off[u]), int(out_off[u + 1])), key=lambda k: int(edges[k]["v2"])) for u in range(V)]
    adj_in = [sorted(int(x) for x in in_nodes[int(in_off[v]):int(in_off[v + 1])]) for v in range(V)]
    for u in range(V):
        t = [int(edges[k]["v2"]) for k in adj_out[u]]
        assert len(t) <= 16 or len(set(t)) == len(t)
    n_store = len(case.seqs)

    def edge_info(v, w):  # getEdgeInfo(v, w, false)
        for k in adj_out[v]:
            if int(edges[k]["v2"]) == w:
                return edges[k]
        raise AssertionError("Edge not found")

    def read_len(r):
        return len(case.seqs[r]) + (len(case.paired[r]) if r in case.paired else 0)

    mol, SE, PE, orc = case.min_overlap_len, case.se_count, case.pe_count, case.original_readcount
    evidence_per_edge, missing_edges, out = {}, [], []

    def find_diff_pos(s1, s2):  # :693-713
        assert len(s1) == len(s2)
        d = []
        for pos in range(len(s1)):
            if s1[pos] != s2[pos]:
                d.append(pos)
                if len(d) == 100:
                    return d
        return d

    def check_read_evidence(contig, startpos, read, index, diff_list):  # :716-743
        true_evidence = False
        read_start = startpos + index
        read_end = i32(read_start + len(read))
        contig_start, contig_end = startpos, i32(startpos + len(contig))
        for d in diff_list:
            if d < read_start or d >= read_end:
                continue
            elif d < contig_start or d >= contig_end:
                continue
            if read[d - read_start] != contig[d - contig_start]:
                true_evidence = False
                break
            else:
                true_evidence = True
        return true_evidence

    def build_diff_list(node1, neighbors, outbranch, missing_inclusion_edges, my_missing):  # :396-535, :537-689
        fwd = bool(case.vertex_fwd[node1])
        sequence_vec, pos_vec, edge_vec, node1_len = [], [], [], 0
        for node in neighbors:
            edge = edge_info(node1, node) if outbranch else edge_info(node, node1)
            r = int(edge["read2"] if outbranch else edge["read1"])
            if r in case.paired:
                raise Failed(BR.BR_PAIRED_NEIGHBOUR)  # :412, :554
            s = case.seqs[r]
            sequence_vec.append(s if fwd else rev_comp(s))  # :414, :556: node1's orientation
            pos_vec.append(int(edge["pos1"]))
            edge_vec.append(edge)
            if not outbranch and node1_len == 0:
                node1_len = read_len(int(edge["read2"]))
        if outbranch:
            startpos_vec = list(pos_vec)
        else:
            max_pos = max(pos_vec)
            startpos_vec = [max_pos - p for p in pos_vec]
        diff_list, distance_vec = [], []
        for i in range(len(neighbors)):
            for j in range(i + 1, len(neighbors)):
                node_i, node_j, seq_i, seq_j = neighbors[i], neighbors[j], sequence_vec[i], sequence_vec[j]
                pos_i, pos_j = startpos_vec[i], startpos_vec[j]
                if node_i == node_j:
                    raise Failed(BR.BR_REPEATED_NEIGHBOUR)  # :446
                if pos_i < pos_j:
                    relative_pos = pos_j - pos_i
                    if relative_pos > i32(len(seq_i) - mol):
                        if not outbranch:
                            raise Failed(BR.BR_BAD_GEOMETRY)  # :605
                        missing_inclusion_edges.append((node_i, node_j))
                        continue
                    if relative_pos > len(seq_i):
                        raise Failed(BR.BR_BAD_GEOMETRY)
                    ln = min(len(seq_i) - relative_pos, len(seq_j))
                    sub_i, sub_j, startpos = seq_i[relative_pos:relative_pos + ln], seq_j[:ln], pos_j
                else:
                    relative_pos = pos_i - pos_j
                    if relative_pos > i32(len(seq_j) - mol):
                        if not outbranch:
                            raise Failed(BR.BR_BAD_GEOMETRY)  # :616
                        missing_inclusion_edges.append((node_j, node_i))
                        continue
                    if relative_pos > len(seq_j):
                        raise Failed(BR.BR_BAD_GEOMETRY)
                    ln = min(len(seq_j) - relative_pos, len(seq_i))
                    sub_i, sub_j, startpos = seq_i[:ln], seq_j[relative_pos:relative_pos + ln], pos_i
                if not outbranch:
                    sub_i, sub_j = sub_i[::-1], sub_j[::-1]
                diff_pos = find_diff_pos(sub_i, sub_j)
                if not ln > 0:
                    raise Failed(BR.BR_BAD_GEOMETRY)  # :471, :625
                for pos in diff_pos:
                    diff_list.append(pos + startpos if outbranch else ln - pos + startpos)  # :473, :627
                if not diff_pos:
                    i_first = pos_i < pos_j or (pos_i == pos_j and node_i < node_j)
                    a, b = (i, j) if i_first else (j, i)
                    which = "2" if outbranch else "1"
                    my_missing.append(dict(score=case.edge_threshold, pos1=relative_pos, pos2=0, ori1=int(edge_vec[a]["ori" + which]),
                                           ori2=int(edge_vec[b]["ori" + which]), ord=ord("-"), read1=int(edge_vec[a]["read" + which]),
                                           read2=int(edge_vec[b]["read" + which]), v1=neighbors[a], v2=neighbors[b],
                                           perc=(100 * ln) // min(len(seq_i), len(seq_j)), len0=ln, len1=ln, len2=0, mismatch_rate=-1.0, pos3=0, pos4=0))
                elif i == 0:
                    if outbranch:
                        distance_vec.append(diff_pos[0] + startpos)
                    else:
                        overlap_len = min(len(seq_i) - pos_vec[i], len(seq_j) - pos_vec[j])  # :600-602
                        distance_vec.append(diff_pos[0] + node1_len - overlap_len)          # :670
        dist = int(0.5 * (min(distance_vec) + max(distance_vec))) if distance_vec else 0  # toward zero
        return sorted(set(diff_list)), dist, sequence_vec, startpos_vec, bool(my_missing)

    def find_branching_evidence(node1, neighbors, outbranch):  # :229-394
        final_branch = [node1] + list(neighbors)
        missing_inclusion_edges, my_missing, stored = [], [], []
        diff_list, dist, sequence_vec, startpos_vec, is_false = build_diff_list(node1, neighbors, outbranch, missing_inclusion_edges, my_missing)
        subreads1 = {x[0] for x in case.dicts[case.vertex_read[node1]]}
        evidence_per_neighbor = {}
        failed = None
        for n, node2 in enumerate(neighbors):
            evidence_list, contig, startpos = [], sequence_vec[n], startpos_vec[n]
            for subread_id, index1, forward in case.dicts[case.vertex_read[node2]]:
                common_subread = subread_id in subreads1
                if subread_id >= SE + PE:
                    subread_id_PE = subread_id - PE
                    common_PE = subread_id_PE in subreads1
                elif subread_id >= SE:
                    subread_id_PE = subread_id + PE
                    common_PE = subread_id_PE in subreads1
                else:
                    subread_id_PE, common_PE = 0, False
                if not common_subread and not common_PE:
                    continue
                if subread_id >= len(case.originals):
                    failed = BR.BR_BAD_ORIGINAL
                    continue
                sequence = case.originals[subread_id] if forward else rev_comp(case.originals[subread_id])
                result1 = common_subread and check_read_evidence(contig, startpos, sequence, index1, diff_list)
                if result1:
                    if not subread_id < 2 * orc:
                        failed = BR.BR_BAD_ORIGINAL  # :300
                    else:
                        evidence_list.append(subread_id)
                result2 = common_PE and check_read_evidence(contig, startpos, sequence, index1, diff_list)  # the sub-read itself again, :304-316
                if result2:
                    joint_id = orc + min(subread_id, subread_id_PE)
                    if not joint_id < 2 * orc:
                        failed = BR.BR_BAD_ORIGINAL  # :319
                    else:
                        evidence_list.append(joint_id)
            evidence_per_neighbor[node2] = sorted(set(evidence_list))
        if failed:
            raise Failed(failed)
        for first, _ in missing_inclusion_edges:  # :328-335
            evidence_per_neighbor[first] = []
            if len(neighbors) == 2:
                final_branch = []
            else:
                final_branch = [x for x in final_branch if x != first]
        it = 1  # :349 (on an empty list: end())
        for neighbor in neighbors:
            if it < len(final_branch) and neighbor == final_branch[it]:
                stored.append((neighbor, evidence_per_neighbor[neighbor]))
                it += 1
        return final_branch[1:], dist, diff_list, is_false, my_missing, stored

    for outbranch in (False, True):
        for node in range(V):
            neighbors = [int(edges[k]["v2"]) for k in adj_out[node]] if outbranch else adj_in[node]
            if len(neighbors) <= 1:
                continue
            rec = dict(node=node, side=int(outbranch), status=BR.BR_OK, is_false=False, dist=0, final=[], diffs=[], n=len(neighbors))
            try:
                final, dist, diffs, is_false, my_missing, stored = find_branching_evidence(node, neighbors, outbranch)
                rec.update(final=final, dist=dist, diffs=diffs, is_false=is_false)
                missing_edges += my_missing
                for neighbor, ev in stored:  # :347-391
                    index = (node, neighbor) if outbranch else (neighbor, node)
                    if index in evidence_per_edge:
                        evidence_per_edge[index] = [x for x in evidence_per_edge[index] if x in ev]
                    else:
                        evidence_per_edge[index] = list(ev)
            except Failed as f:
                rec["status"] = f.status
            out.append(rec)
    return dict(branches=out, evidence=evidence_per_edge, missing=missing_edges)


MISSING_FIELDS = ("score", "mismatch_rate", "pos1", "pos2", "pos3", "pos4", "ori1", "ori2", "ord", "read1", "read2", "v1", "v2", "perc", "len0", "len1", "len2")


def as_expected(res):
    """a BranchEvidence in the shape restate() returns, every field of every table"""
    branches = []
    n_nb = n_diff = 0
    for b, r in enumerate(res.branches):
        assert int(r["nb_first"]) == n_nb and int(r["diff_first"]) == n_diff and int(r["pad"]) == 0, "the ranges are not back to back"
        n_nb += int(r["nb_count"])
        n_diff += int(r["diff_count"])
        branches.append(dict(node=int(r["node"]), side=int(r["side"]), status=int(r["status"]), is_false=bool(r["is_false"]), dist=int(r["dist"]),
                             final=res.neighbours(b).tolist(), diffs=res.diffs(b).tolist(), n=int(r["n_neighbours"])))
    assert n_nb == res.branch_nb.size and n_diff == res.diff_pos.size
    assert int(res.ev_off[0]) == 0 and int(res.ev_off[-1]) == res.ev_ids.size
    keys = [tuple(int(x) for x in e) for e in res.ev_edge]
    assert keys == sorted(set(keys)), "ev_edge is not in strictly ascending (u, v)"
    missing = [{k: (float(m[k]) if k in ("score", "mismatch_rate") else int(m[k])) for k in MISSING_FIELDS} for m in res.missing_edges]
    assert all(int(m["pad"]) == 0 and int(m["_p2"]) == 0 for m in res.missing_edges)
    return dict(branches=branches, evidence=res.evidence(), missing=missing)


def check_counts(res, want):
    c = res.counts
    assert c["n_branches"] == len(want["branches"]) and c["n_branch_nb"] == res.branch_nb.size and c["n_diff"] == res.diff_pos.size
    assert c["n_ev_edges"] == len(want["evidence"]) and c["n_ev_ids"] == res.ev_ids.size and c["n_missing"] == len(want["missing"])
    assert c["n_failed"] == sum(b["status"] != BR.BR_OK for b in want["branches"])
    assert c["some_failed"] == (c["n_failed"] > 0)


def assert_same_tables(a, b):
    """two BranchEvidence, table by table and status by status"""
    for k in ("branches", "branch_nb", "diff_pos", "ev_edge", "ev_off", "ev_ids", "missing_edges"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    for k in ("n_branches", "n_branch_nb", "n_diff", "n_ev_edges", "n_ev_ids", "n_missing", "n_items", "n_failed", "some_failed"):
        assert a.counts[k] == b.counts[k], k


# ---- the seeded maker ------------------------------------------------------------------------------------------------------------------

def make_case(seed, n_contigs=40, genome_len=420, n_haps=3, n_orig_se=30, n_orig_pe=40, reverse=False, garbage=0, max_out=3, name=None, island_step=60,
              cap_pair=False, bubbles=0):
    """A genome with islands of haplotype variants between conserved stretches; contigs cut from the haplotypes; an edge u -> v where v starts
    inside u and the two agree on their overlap (a real overlap), at most max_out per vertex, a contained v included; original reads (singles,
    then /1 mates, then /2 mates) cut from the haplotypes, in the dict of every contig of their haplotype they overlap by 8 bases or
    more — also where they start a few bases before the contig (a negative index1).  reverse: every vertex is a reverse one and the store
    holds the reverse complements.  garbage: that many contigs are random sequence.  cap_pair: three more contigs, u -> (v1, v2) with v2 random over
    160 bases: a pair that reaches the 100-position cap.  Half of the mate pairs have /2 ahead of /1.  bubbles: that many times four contigs on a
    170-base genome of their own with two haplotypes that differ in [15, 35) and [105, 125): u = hap0[0:100], u' = hap1[10:95], v = hap0[40:160],
    v' = hap1[45:150] with u -> v, u -> v', u' -> v, and three single-end originals of hap0, [85, 130), [20, 60) and [25, 115), in the dicts of u and v:
    the edge (u, v) is stored from the out-branch u (the first and the third original) and from the in-branch v (the second and the third)."""
    rng = np.random.default_rng(seed)
    base = "".join(rng.choice(list("ACGT"), genome_len))
    haps = []
    for h in range(n_haps):
        s = list(base)
        for island in range(40, genome_len - 20, island_step):
            for p in range(island, island + 20):
                if rng.random() < 0.3:
                    s[p] = "ACGT"[("ACGT".index(base[p]) + 1 + h) % 4]
        haps.append("".join(s))
    contigs = []
    for c in range(n_contigs):
        h, ln = int(rng.integers(n_haps)), int(rng.integers(25, 130))
        s = int(rng.integers(0, genome_len - ln))
        seq = haps[h][s:s + ln] if c >= garbage else "".join(rng.choice(list("ACGT"), ln))
        contigs.append((h, s, s + ln, seq))
    contigs.sort(key=lambda x: (x[1], x[2]))
    if cap_pair:
        contigs += [(0, 10, 180, haps[0][10:180]), (0, 15, 185, haps[0][15:185]), (0, 16, 176, "".join(rng.choice(list("ACGT"), 160)))]
    motif = []  # (first vertex, hap0)
    for _ in range(bubbles):
        b0 = "".join(rng.choice(list("ACGT"), 170))
        b1 = "".join("ACGT"[("ACGT".index(c) + 1) % 4] if (15 <= p < 35 or 105 <= p < 125) and p % 3 == 0 else c for p, c in enumerate(b0))
        motif.append((len(contigs), b0))
        contigs += [(-1, 0, 100, b0[0:100]), (-1, 10, 95, b1[10:95]), (-1, 40, 160, b0[40:160]), (-1, 45, 150, b1[45:150])]
    V = len(contigs)
    perm = [int(x) for x in rng.permutation(V)]  # vertex -> read
    edges = []
    for u, (hu, su, eu, sequ) in enumerate(contigs[:n_contigs]):
        cand = []
        for v, (hv, sv, ev, seqv) in enumerate(contigs[:n_contigs]):
            if v == u or not (su < sv < eu):
                continue
            n = min(eu, ev) - sv
            if n >= 12 and (sequ[sv - su:sv - su + n] == seqv[:n] or rng.random() < 0.05):
                cand.append((v, sv - su))
        rng.shuffle(cand)
        edges += [(u, v, pos) for v, pos in cand[:max_out]]
    if cap_pair:
        edges += [(n_contigs, n_contigs + 1, 5), (n_contigs, n_contigs + 2, 6)]
    for first, _ in motif:
        edges += [(first, first + 2, 40), (first, first + 3, 45), (first + 1, first + 2, 30)]
    SE, PE = n_orig_se + 3 * bubbles, n_orig_pe
    origs = [None] * (SE + 2 * PE)  # (hap, start, seq as stored, forward)
    def cut(h, s, ln):
        fwd = rng.random() < 0.7
        seq = haps[h][s:s + ln]
        return (h, s, seq if fwd else rev_comp(seq), int(fwd))
    for k in range(n_orig_se):
        ln = int(rng.integers(25, 45))
        origs[k] = cut(int(rng.integers(n_haps)), int(rng.integers(0, genome_len - ln)), ln)
    for k in range(PE):
        h, l1, l2, gap = int(rng.integers(n_haps)), int(rng.integers(25, 40)), int(rng.integers(25, 40)), int(rng.integers(0, 40))
        s = int(rng.integers(0, genome_len - l1 - l2 - gap))
        if rng.random() < 0.5:
            origs[SE + k], origs[SE + PE + k] = cut(h, s, l1), cut(h, s + l1 + gap, l2)
        else:
            origs[SE + PE + k], origs[SE + k] = cut(h, s, l2), cut(h, s + l2 + gap, l1)
    motif_entries = []
    for m, (first, b0) in enumerate(motif):
        for k, (a, b) in enumerate(((85, 130), (20, 60), (25, 115))):
            oid, fwd = n_orig_se + 3 * m + k, int(rng.random() < 0.7)
            origs[oid] = (-100, a, b0[a:b] if fwd else rev_comp(b0[a:b]), fwd)
            motif_entries += [(first, (oid, a, fwd)), (first + 2, (oid, a - 40, fwd))]
    dicts = [None] * V
    for v, (h, s, e, _) in enumerate(contigs):
        d = []
        for oid, (oh, os_, oseq, ofwd) in enumerate(origs):
            if oh == h and min(e, os_ + len(oseq)) - max(s, os_) >= 8 and os_ >= s - 6 and rng.random() < 0.85:
                d.append((oid, os_ - s, ofwd))
        dicts[perm[v]] = d
    for v, entry in motif_entries:
        dicts[perm[v]] = sorted(dicts[perm[v]] + [entry])
    seqs = [None] * V
    for v, c in enumerate(contigs):
        seqs[perm[v]] = rev_comp(c[3]) if reverse else c[3]
    return Case(name or f"seed{seed}", seqs, perm, [0 if reverse else 1] * V, edges, dicts, [o[2] for o in origs], SE, PE, SE + PE)


# ---- recorded reference vectors --------------------------------------------------------------------------------------------------------

def golden_cases():
    """[(Case, want in restate()'s shape)] from tests/golden/branch_evidence.json, every recorded field"""
    import json
    import os

    data = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "branch_evidence.json")))
    out = []
    for c in data["cases"]:
        case, w = Case.from_json(c["inputs"]), c["want"]
        false_sets = (set(w["false_in"]), set(w["false_out"]))
        branches = [dict(node=x["node"], side=x["side"], status=BR.BR_OK, is_false=x["node"] in false_sets[x["side"]], dist=x["dist"],
                         final=x["final_branch"][1:], diffs=x["diffs"], n=x["n"]) for x in w["calls"]]
        assert all(not x["final_branch"] or x["final_branch"][0] == x["node"] for x in w["calls"])
        missing = [dict(zip(data["missing_keys"], m), pos3=0, pos4=0) for m in w["missing"]]
        for m in missing:
            m["score"], m["mismatch_rate"] = float(m["score"]), float(m["mismatch_rate"])
        out.append((case, dict(branches=branches, evidence={(u, v): ids for u, v, ids in w["evidence"]}, missing=missing)))
    return out, data


# ---- hand-built cases ------------------------------------------------------------------------------------------------------------------

def extend(case, seqs, fwd, edges, dicts=None, paired=None, name=None):
    """`case` with len(seqs) more vertices (vertex V + i is read R + i) and more edges (vertex ids of the extended graph)"""
    import copy

    c = copy.deepcopy(case)
    V, R = c.n_vertices, len(c.seqs)
    c.seqs += list(seqs)
    c.vertex_read += [R + i for i in range(len(seqs))]
    c.vertex_fwd += list(fwd)
    c.edges += list(edges)
    c.dicts += [sorted(d) for d in (dicts or [[] for _ in seqs])]
    for i, s in (paired or {}).items():
        c.paired[R + i] = s
    c.name = name or c.name
    assert len(c.dicts) == len(c.seqs) and V + len(seqs) == c.n_vertices
    return c


def random_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def mutate(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def status_cases():
    """{name: (Case, {(node, side): status})}: a bubble that stays HC_BR_OK beside one branch (or two) built for each status"""
    rng = np.random.default_rng(77)
    base = make_case(5, n_contigs=0, n_orig_se=2, n_orig_pe=1, bubbles=1)  # 4 vertices, 7 originals
    V = base.n_vertices
    a, b, c = random_seq(rng, 60), random_seq(rng, 60), random_seq(rng, 60)
    out = {}
    # a paired neighbour: the read of V + 2 has two sequences
    out["paired"] = (extend(base, [a, b, c], [1, 1, 1], [(V, V + 1, 10), (V, V + 2, 12)], paired={2: "ACGTACGT"}), {(V, 1): BR.BR_PAIRED_NEIGHBOUR})
    # a repeated target: both the out-branch V and the in-branch V + 1 see the pair twice
    out["repeated"] = (extend(base, [a, b, c], [1, 1, 1], [(V, V + 1, 10), (V, V + 2, 11), (V, V + 1, 12)]),
                       {(V, 1): BR.BR_REPEATED_NEIGHBOUR, (V + 1, 0): BR.BR_REPEATED_NEIGHBOUR})
    # relative_pos == size with min_overlap_len == 0: len is 0
    z = extend(base, [a, b[:20], c], [1, 1, 1], [(V, V + 1, 5), (V, V + 2, 25)])
    z.min_overlap_len = 0
    out["len_zero"] = (z, {(V, 1): BR.BR_BAD_GEOMETRY})
    # an in-branch whose pair would be a missing inclusion pair
    out["in_inclusion"] = (extend(base, [a[:40], b, c], [1, 1, 1], [(V, V + 2, 50), (V + 1, V + 2, 0)]), {(V + 2, 0): BR.BR_BAD_GEOMETRY})
    # an id beyond the originals in both dicts
    n_orig = len(base.originals)
    out["beyond_originals"] = (extend(base, [a, a[10:] + b[:10], mutate(a[12:] + c[:12], [20])], [1, 1, 1], [(V, V + 1, 10), (V, V + 2, 12)],
                                      dicts=[[(n_orig + 3, 0, 1)], [(n_orig + 3, 0, 1)], []]), {(V, 1): BR.BR_BAD_ORIGINAL})
    # the assert of :300: evidence whose id is not below 2 * original_readcount
    y = extend(base, [a, a[10:] + b[:10], mutate(a[12:] + c[:12], [20])], [1, 1, 1], [(V, V + 1, 10), (V, V + 2, 12)])
    o = n_orig - 1  # the last original (a /2 mate), re-used as a read that covers the difference
    y.originals[o] = y.seqs[len(base.seqs) + 1][:40]
    y.dicts[len(base.seqs)] = [(o, 10, 1)]
    y.dicts[len(base.seqs) + 1] = [(o, 0, 1)]
    y.original_readcount = 3  # 2 * 3 = 6 is not above the id 6
    out["assert_300"] = (y, {(V, 1): BR.BR_BAD_ORIGINAL})
    return out


def fan_case(seed, fans, name="fans", **kw):
    """Branches of explicit shape.  fans: dicts with side ("out" / "in"), k neighbours, overlap L (every pair compares L positions), diffs: per
    neighbour j > 0 the positions (in the compared order: from the front for an out-branch, from the back for an in-branch) where it differs
    from neighbour 0, dict_sizes per neighbour, fwd (node1's orientation; the neighbours' stored bytes follow it), shift: neighbour j starts
    shift * j later (out-branch only).  Every neighbour's originals are cut from it (some with one base changed at a difference), listed in
    node1's dict too; they are single-end, a few of them /1 or /2 mates whose mate is in node1's dict instead."""
    rng = np.random.default_rng(seed)
    seqs, fwd, edges, dicts, originals = [], [], [], [], []
    n_se = sum(sum(f.get("dict_sizes", [0] * f["k"])) for f in fans)
    for f in fans:
        k, L, out, node_fwd = f["k"], f["L"], f.get("side", "out") == "out", f.get("fwd", 1)
        shift = f.get("shift", 0)
        node1 = len(seqs)
        common = random_seq(rng, L + shift * k)
        seqs.append(random_seq(rng, 30) + common[:10] if out else common[-10:] + random_seq(rng, 30))
        fwd.append(node_fwd)
        dicts.append([])
        for j in range(k):
            d = f.get("diffs", [[]] * k)[j] if j else []
            s = common[shift * j:shift * j + L] if out else common[:L]
            s = mutate(s, d if out else [L - 1 - p for p in d])
            v = len(seqs)
            seqs.append(s if node_fwd else rev_comp(s))
            fwd.append(1)
            dicts.append([])
            edges.append((node1, v, 30 + shift * j) if out else (v, node1, L - 10))
            for _ in range(f.get("dict_sizes", [0] * k)[j]):
                oid = len(originals)
                ln = int(rng.integers(1, min(L, 40) + 1)) if rng.random() < 0.8 else L
                at = int(rng.integers(0, L - ln + 1))
                o = s[at:at + ln]
                if rng.random() < 0.3 and ln > 1:
                    o = mutate(o, [int(rng.integers(ln))])
                ofwd = int(rng.random() < 0.6)
                originals.append(o if ofwd else rev_comp(o))
                dicts[v].append((oid, at, ofwd))
                dicts[node1].append((oid, 0, ofwd))
    return Case(name, seqs, list(range(len(seqs))), fwd, edges, [sorted(d) for d in dicts], originals, len(originals), 0, max(len(originals), 1), **kw)


def paired_then_bad_read():
    """(Case, graph): an out-branch whose FIRST neighbour is paired and whose SECOND neighbour's record names a read outside the store: the
    call refuses the arguments (every neighbour's reads are checked ahead of any status), device and mirror alike"""
    rng = np.random.default_rng(78)
    base = make_case(5, n_contigs=0, n_orig_se=2, n_orig_pe=1, bubbles=1)
    V = base.n_vertices
    case = extend(base, [random_seq(rng, 60) for _ in range(3)], [1, 1, 1], [(V, V + 1, 10), (V, V + 2, 12)], paired={1: "ACGTACGT"})
    g = case.graph()
    k = int(np.flatnonzero((g["edges"]["v1"] == V) & (g["edges"]["v2"] == V + 2))[0])
    g["edges"]["read2"][k] = len(case.seqs) + 5
    return case, g

