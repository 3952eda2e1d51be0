"""The host mirror of OverlapGraph::writeGraphToFile / writeDiGraphToFile / write2GFA (hc_host_graph_write_text) against the
reference's own three functions (tests/golden/graph_files.json, made by tests/golden/make_golden_graph_files.py), byte for byte
and with the counts.  The reference's asserts cannot be recorded by the probe (the process aborts): for them the mirror's status
and the reported place — the first in file order — are checked."""
import ctypes as C

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import host
from tests import _graph_text as GT
from tests import _trans

CASES = GT.load_cases()
HC_ERR_ARG = -1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_equals_reference(case):
    g = GT.mirror(GT.case_graph(case))
    bases, off, first = GT.raw_reads(case["reads"])
    for kind in GT.KINDS:
        text, counts = host.graph_write_text(g, kind, bases=bases, seq_off=off, read_first_seq=first, **GT.settings_of(case))
        assert text == case["expected"][GT.EXPECTED[kind]].encode(), (case["name"], kind)
        GT.check_counts(counts, case, kind, text, (case["name"], kind))


def test_golden_covers_what_the_issue_lists():
    names = {c["name"] for c in CASES}
    assert {"reverse_pair", "repeated", "first_copy_zero", "first_copy_positive", "inclusion_vertex", "paired_reads", "duplicates", "perc",
            "digit_boundaries", "edgeless"} <= names
    by = {c["name"]: c for c in CASES}
    assert by["first_copy_zero"]["expected"]["n_pairs"] == 3 and by["first_copy_positive"]["expected"]["n_pairs"] == 2
    assert "9,10\n10,9\n" in by["digit_boundaries"]["expected"]["graph_txt"] and "99\t100\n" in by["digit_boundaries"]["expected"]["digraph_txt"]
    assert any(c["expected"]["c_count"] and c["expected"]["l_count"] for c in CASES)
    assert by["edgeless"]["expected"]["graph_txt"] == "5\n0\n" and by["edgeless"]["expected"]["digraph_txt"] == ""


def _graph(V, pairs, incl=None, **fields):
    r = _trans.make_records(np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64), 1)
    r["score"], r["mismatch_rate"] = 0.99, 0.0
    for k, v in fields.items():
        r[k] = v
    return (*_trans.csr_from_inserts(r, V), np.zeros(V, np.uint8) if incl is None else np.array(incl, np.uint8))


def _status(g, kind, reads=None, n_singles=0, **kw):
    bases, off, first = GT.raw_reads(reads or [])
    text, c = host.graph_write_text(GT.mirror(g), kind, bases=bases, seq_off=off, read_first_seq=first, n_singles=n_singles, **kw)
    assert text == b"" and c["n_bytes"] == 0 and c["n_lines"] == 0
    return N.GRAPH_TEXT_STATUS[c["status"]], c["bad_v"], c["bad_pos"]


SIX = [["ACGTN", "", 0], ["A", "", 0], ["CCGT", "", 0], ["GGA", "", 0], ["TTTT", "", 0], ["ACG", "", 0]]


def test_self_loop_is_reported_first_in_file_order():
    """hc_host_graph_adopt takes a self-loop; two are planted and the earlier record is reported, in every kind."""
    g = _graph(6, [(0, 1), (2, 3), (2, 2), (4, 4), (2, 5)])
    for kind in GT.KINDS:
        assert _status(g, kind, SIX, 6) == ("SELF_LOOP", 2, 1), kind


def test_non_empty_inclusion_list():
    g = _graph(6, [(0, 1), (3, 4), (3, 5), (5, 0)], incl=[0, 0, 0, 1, 0, 1])
    assert _status(g, "cliques") == ("INCLUSION_HAS_EDGES", 3, 0)
    # the two other writers do not look at the bits
    text, c = host.graph_write_text(GT.mirror(g), "digraph")
    assert text == b"0\t1\n3\t4\n3\t5\n5\t0\n" and c["status"] == 0


def test_weak_reverse_edge():
    """checkEdge's assert fires on the first 1 -> 3 record, whatever comes behind it, when 3 -> 1 is written."""
    pairs = [(0, 1), (1, 3), (1, 3), (3, 0), (3, 1), (4, 0)]
    g = _graph(6, pairs, score=[0.99, 0.5, 0.99, 0.99, 0.99, 0.99], mismatch_rate=[0, 0.2, 0, 0, 0, 0])
    assert _status(g, "cliques", edge_threshold=0.9, merge_contigs=0.1) == ("WEAK_EDGE", 3, 1)
    text, c = host.graph_write_text(GT.mirror(g), "cliques", edge_threshold=0.9, merge_contigs=0.2)  # the mismatch rate saves it
    assert c["status"] == 0 and text.startswith(b"6\n")
    # an earlier self-loop wins over it, a later one does not
    g2 = _graph(6, pairs + [(2, 2)], score=[0.99, 0.5, 0.99, 0.99, 0.99, 0.99, 0.99], mismatch_rate=[0, 0.2, 0, 0, 0, 0, 0])
    assert _status(g2, "cliques", edge_threshold=0.9, merge_contigs=0.1) == ("SELF_LOOP", 2, 0)
    g3 = _graph(6, pairs + [(5, 5)], score=[0.99, 0.5, 0.99, 0.99, 0.99, 0.99, 0.99], mismatch_rate=[0, 0.2, 0, 0, 0, 0, 0])
    assert _status(g3, "cliques", edge_threshold=0.9, merge_contigs=0.1) == ("WEAK_EDGE", 3, 1)


def test_gfa_read_asserts():
    g = _graph(6, [(0, 1), (1, 2), (4, 5)])
    paired = [r[:] for r in SIX]
    paired[2] = ["CCGT", "AAC", 1]
    assert _status(g, "gfa", paired, 6) == ("PAIRED_IN_SINGLES", 2, 0)
    assert host.graph_write_text(GT.mirror(g), "gfa", n_singles=2, **dict(zip(("bases", "seq_off", "read_first_seq"), GT.raw_reads(paired))))[1]["status"] == 0
    empty = [r[:] for r in SIX]
    empty[3][0] = ""
    empty[4][0] = ""
    assert _status(g, "gfa", empty, 6) == ("EMPTY_SEQ", 3, 0)


def test_bad_base_in_a_reversed_read_only():
    """build_rev_comp exits on the byte; the read as stored is written as it is."""
    reads = [["ACXT", "", 0], ["ACGT", "", 0], ["AC-T", "", 0]]
    g = _graph(6, [(0, 1), (3, 4)])
    bases, off, first = GT.raw_reads(reads)
    text, c = host.graph_write_text(GT.mirror(_graph(3, [(0, 1)])), "gfa", n_singles=3, bases=bases, seq_off=off, read_first_seq=first)
    assert c["status"] == 0 and b"S\t0\tACXT\n" in text and b"S\t2\tAC-T\n" in text
    assert _status(g, "gfa", reads, 3) == ("BAD_BASE", 3, 0)


def test_cap_and_refusals():
    case = next(c for c in CASES if c["name"] == "random_singles")
    g = GT.mirror(GT.case_graph(case))
    st = N.hc_graph_text_settings(case["edge_threshold"], case["merge_contigs"], 0)
    c = N.hc_graph_text_counts()
    want = case["expected"]["graph_txt"].encode()
    buf = np.zeros(len(want), np.uint8)
    assert N.lib.hc_host_graph_write_text(g._h, 0, C.byref(st), None, None, None, 0, buf.ctypes.data, len(want) - 1, C.byref(c)) == HC_ERR_ARG
    assert c.n_bytes == len(want) and c.n_pairs == case["expected"]["n_pairs"] and not buf.any()
    assert N.lib.hc_host_graph_write_text(g._h, 0, C.byref(st), None, None, None, 0, buf.ctypes.data, len(want), C.byref(c)) == 0
    assert buf.tobytes() == want
    assert N.lib.hc_host_graph_write_text(g._h, 3, C.byref(st), None, None, None, 0, None, 0, C.byref(c)) == HC_ERR_ARG
    assert N.lib.hc_host_graph_write_text(g._h, 0, None, None, None, None, 0, None, 0, C.byref(c)) == HC_ERR_ARG
    assert N.lib.hc_host_graph_write_text(g._h, 2, C.byref(st), None, None, None, 0, None, 0, C.byref(c)) == HC_ERR_ARG  # GFA without reads
    bases, off, first = GT.raw_reads(case["reads"])
    st.n_singles = len(case["reads"]) + 1
    assert N.lib.hc_host_graph_write_text(g._h, 2, C.byref(st), bases.ctypes.data, off.ctypes.data, first.ctypes.data, len(case["reads"]), None, 0,
                                          C.byref(c)) == HC_ERR_ARG


def test_widest_len0():
    """std::to_string(int) at the top of the range.  The mirror's Edge, like the reference's, derives len0 = len1 + len2 with len1 > 0
    (Edge::set_len), so a negative len0 exists only in a record handed to the device: tests/test_gpu_graph_text.py pins that text."""
    g = _graph(12, [(9, 10), (10, 11)], len1=[2147483647, 1], len2=[0, 0], perc=[100, 5])
    bases, off, first = GT.raw_reads(GT.random_reads([3] * 12, 3))
    text, c = host.graph_write_text(GT.mirror(g), "gfa", n_singles=12, bases=bases, seq_off=off, read_first_seq=first)
    assert b"L\t9\t+\t10\t+\t2147483647M\n" in text and b"L\t10\t+\t11\t+\t1M\n" in text
    assert (c["l_count"], c["c_count"]) == (1, 1)
