"""Shared by the graph-text tests (graph.txt / digraph.txt / GFA): the cases of tests/golden/graph_files.json as graphs and raw read
arrays, the host mirror's run of a kind, and seeded graphs and reads."""
import json
import os

import numpy as np

from haploconduct_amd import _native as N
from haploconduct_amd.host import EDGE_DTYPE
from tests import _trans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_files.json")
KINDS = ("cliques", "digraph", "gfa")
EXPECTED = {"cliques": "graph_txt", "digraph": "digraph_txt", "gfa": "gfa"}
STATUS = {name: k for k, name in enumerate(N.GRAPH_TEXT_STATUS)}


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def golden_records(edges_in):
    """The full records of a case's input edges (the encoding of make_golden_graph_files.py)."""
    r = np.zeros(len(edges_in), EDGE_DTYPE)
    for k, (v1, v2, r1, r2, p1, p2, l1, l2, o1, o2, od, score, mm, perc) in enumerate(edges_in):
        r[k] = (score, mm, p1, p2, 0, 0, o1, o2, od, 0, r1, r2, 0, v1, v2, perc, l1 + l2, l1, l2)
    return r


def raw_reads(reads):
    """(bases, seq_off, read_first_seq) of a read table [seq1, seq2, paired]: the raw arrays hc_set_reads takes."""
    seqs, first = [], [0]
    for s1, s2, p in reads:
        seqs.append(s1)
        if p:
            seqs.append(s2)
        first.append(len(seqs))
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer("".join(seqs).encode(), np.uint8).copy(), off, np.array(first, np.uint32)


def case_graph(case):
    """(edges, out_off, in_nodes, in_off, inclusions) of a golden case: what its addEdge calls leave."""
    return (*_trans.csr_from_inserts(golden_records(case["edges_in"]), case["V"]), np.array(case["inclusions"], np.uint8))


def mirror(graph):
    edges, out_off, in_nodes, in_off, incl = graph
    return _trans.Mirror(edges, out_off, in_nodes, in_off, incl).g


def settings_of(case):
    return dict(edge_threshold=case["edge_threshold"], merge_contigs=case["merge_contigs"], n_singles=case["n_singles"])


def check_counts(counts, case, kind, text, where):
    exp = case["expected"]
    assert counts["status"] == 0, (where, counts)
    assert counts["n_bytes"] == len(text), (where, counts)
    assert counts["n_lines"] == text.count(b"\n"), (where, counts)
    if kind == "cliques":
        assert counts["n_pairs"] == exp["n_pairs"], (where, counts)
    if kind == "gfa":
        assert (counts["n_segments"], counts["l_count"], counts["c_count"]) == (exp["n_segments"], exp["l_count"], exp["c_count"]), (where, counts)


def random_reads(lengths, seed, alphabet="ACGTN"):
    """Single-end reads of the given lengths as a read table."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet.encode(), np.uint8)
    return [[letters[rng.integers(0, len(letters), n)].tobytes().decode(), "", 0] for n in lengths]


def records_for(v1, v2, seed):
    """Records in insertion order for the pairs: scores on both sides of 0 that all pass checkEdge's assert at edge_threshold 0.9 /
    merge_contigs 0.05, perc of 100 and below, len0 = len1 + len2 of one to ten digits (the mirror's Edge derives it: Edge::set_len)."""
    rng = np.random.default_rng(seed)
    r = _trans.make_records(np.asarray(v1), np.asarray(v2), seed)
    n = r.shape[0]
    r["score"] = rng.choice([0.99, 0.95, 0.5, 0.0, -1.0], n)
    r["mismatch_rate"] = np.where(r["score"] < 0.9, 0.0, rng.choice([0.0, 0.02, 0.3], n))
    r["perc"] = rng.choice([100, 99, 60], n)
    r["len1"], r["len2"] = rng.choice([1, 9, 10, 150, 99999, 2147483647], n), 0
    r["len0"] = r["len1"]
    return r
