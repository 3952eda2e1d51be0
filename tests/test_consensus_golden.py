"""Super-read consensus on the host (include/hcsr.h: hc_host_sr_consensus and its helpers) against vectors produced by the
reference's own SRBuilder::consensus / consensus_pos (tests/golden/make_golden_consensus.py: probe with substitutes)."""
import numpy as np
import pytest

from haploconduct_amd import HcError
from haploconduct_amd import consensus as SR
from haploconduct_amd import host
from haploconduct_amd.readstore import ReadSet
from tests import _sr


def _mirror(reads, layouts, members, min_qual, mcs, ec, sub, n_threads=1):
    return host.sr_consensus(reads, layouts, members, min_qual, mcs, ec, sub, n_threads=n_threads)


def test_mirror_equals_every_golden_case():
    assert _sr.check_against_golden(_mirror) >= 150


def test_mirror_threads_give_the_same_bytes():
    reads, cases, index = _sr.load_golden()
    layouts, members = _sr.case_arrays(cases, index)
    layouts, members = np.tile(layouts, 40), members  # many layouts over the same members: several blocks per thread
    a = _mirror(reads, layouts, members, 0.99, 2, 1, 0, n_threads=1)
    b = _mirror(reads, layouts, members, 0.99, 2, 1, 0, n_threads=7)
    _sr.assert_same(a, b, "1 thread vs 7")


def test_golden_covers_what_the_contract_names():
    _, cases, _ = _sr.load_golden()
    st = {c["status"] for c in cases}
    assert {SR.SR_OK, SR.SR_NO_SUPPORT, SR.SR_MEMBER_SHORT, SR.SR_UNCOVERED} <= st
    depths = {len(c["members"]) for c in cases}
    assert {1, 2, 3, 8, 40} <= depths
    quals = "".join(c["cons_qual"] for c in cases)
    assert "~" in quals and "$" in quals
    assert {c["settings"]["min_qual"] for c in cases} >= {0.9, 0.99} and {c["settings"]["min_clique_size"] for c in cases} >= {2, 4}


def test_two_member_table_equals_direct_evaluation():
    """Every entry of the table the device reads one- and two-member columns from, for a 42-value alphabet, against
    consensus_pos evaluated directly on the two (base, quality) strings."""
    K = 42
    bases = b"ACGTN"
    for min_qual in (0.99, 0.9):
        t = SR.table(min_qual, K)

        def want(nuc, qual):
            r = SR.column(nuc, qual, min_qual)
            assert r is not None
            return 255 if r[0] == ord("N") else r[1] - 33

        n = 0
        for b1 in range(5):
            for q1 in range(K if b1 < 4 else 1):
                assert t[25 * 128 * 128 + b1 * 128 + q1] == want(bases[b1:b1 + 1], bytes([q1 + 33])), (b1, q1)
                for b2 in range(5):
                    for q2 in range(K if b2 < 4 else 1):
                        got = t[((b1 * 5 + b2) * 128 + q1) * 128 + q2]
                        assert got == want(bases[b1:b1 + 1] + bases[b2:b2 + 1], bytes([q1 + 33, q2 + 33])), (b1, q1, b2, q2)
                        n += 1
        assert n >= 16 * K * K  # (K + 1)^2 * 2 entries and the base-dependent ones on top


def test_column_tie_order_and_clamp():
    assert SR.column(b"TA", b"55", 0.3)[0] == ord("A")  # A, T, C, G
    assert SR.column(b"GC", b"55", 0.3)[0] == ord("C")
    assert SR.column(b"GT", b"55", 0.3)[0] == ord("T")
    assert SR.column(b"AAA", b"III", 0.99) == (ord("A"), ord("~"))  # Phred 93
    assert SR.column(b"N", b"I", 0.99) == (ord("N"), ord("$"))
    assert SR.column(b"AC", b"##", 0.99) == (ord("N"), ord("$"))  # minQual applies from two members on
    assert SR.column(b"A", b"#", 0.99)[0] == ord("A")  # ... and not to one


def _reads():
    return ReadSet.from_lists([("ACGTACGTAC", "IIIIIIIIII"), ("CGTACGTACG", "5555555555"), ("ACGTA", "IIIII")],
                              [(("ACGTACGT", "IIIIIIII"), ("TTTTCCCC", "55555555"))])


def _one(reads, members, total_len, **kw):
    m = np.array([(r, p, s, v, (0, 0)) for r, s, v, p in members], SR.SR_MEMBER_DTYPE)
    lay = np.array([(0, len(members), total_len)], SR.SR_LAYOUT_DTYPE)
    return host.sr_consensus(reads, lay, m, **kw)


@pytest.mark.parametrize("members,total_len", [
    ([(7, 0, 0, 0)], 10),                       # read index out of range
    ([(0, 0, 0, 1)], 11),                       # first position not 0
    ([(0, 0, 0, 0), (1, 0, 0, 5), (2, 0, 0, 3)], 15),  # positions not ascending
    ([(0, 0, 0, 0), (1, 0, 0, 5)], 14),         # total_len shorter than a member's end
    ([(0, 1, 0, 0)], 10),                       # mate of a single-end read
    ([(3, 0, 0, 0)], 10),                       # get_seq(0) of a pair
    ([(0, 0, 2, 0)], 10),                       # rev > 1
    ([(0, 3, 0, 0)], 10),                       # no such sequence
    ([], 10),                                   # no member
    ([(0, 0, 0, 0)], -1),                       # negative total_len
])
def test_malformed_layouts_are_refused(members, total_len):
    r = _one(_reads(), members, total_len)
    assert int(r.status[0]) == SR.SR_BAD_LAYOUT and int(r.ret[0]) == 0 and r.cons_seq.size == 0


def test_member_range_of_a_layout_is_checked():
    reads = _reads()
    m = np.array([(0, 0, 0, 0, (0, 0))], SR.SR_MEMBER_DTYPE)
    for first, n in ((1, 1), (0, 2), (2**63, 1), (0, 2**32 - 1)):
        lay = np.array([(first, n, 10)], SR.SR_LAYOUT_DTYPE)
        r = host.sr_consensus(reads, lay, m)
        assert int(r.status[0]) == SR.SR_BAD_LAYOUT


def test_pairs_and_orientations_through_the_mirror():
    reads = _reads()
    r = _one(reads, [(3, 1, 0, 0), (3, 2, 1, 0)], 8, min_qual=0.5)  # /1 forward over the reverse complement of /2 (GGGGAAAA)
    assert int(r.status[0]) == SR.SR_OK and r.cons_seq.size == 8


def test_invalid_symbols_are_reported():
    reads = ReadSet.from_lists([("ACGTXCGT", "IIIIIIII"), ("ACGTACGT", "IIII\x1fIII")])
    for k in (0, 1):
        r = _one(reads, [(k, 0, 0, 0)], 8)
        assert int(r.status[0]) == SR.SR_BAD_SYMBOL and int(r.ret[0]) == 0 and r.cons_seq.size == 0


def test_edge_layouts_follow_sort_vertices():
    reads = ReadSet.from_lists([("A" * 10, "I" * 10), ("C" * 12, "I" * 12), ("G" * 8, "I" * 8)], [(("ACGT", "IIII"), ("ACGT", "IIII"))])
    e = np.zeros(4, host.EDGE_DTYPE)
    # (read1, read2, v1, v2, ori1, ori2, pos1)
    rows = [(0, 1, 0, 1, 1, 1, 4),    # base = read 0 (vertex 0), the other at +4
            (1, 0, 5, 0, 0, 1, 3),    # base = read 0 (the smaller vertex is v2), read 1 at -3, reverse vertex
            (2, 0, 2, 4, 1, 0, 0),    # new_pos = 0: the other member goes in front of the base
            (0, 2, 0, 2, 1, 1, 1)]    # the other member lies inside the base
    for i, (r1, r2, v1, v2, o1, o2, p) in enumerate(rows):
        e[i]["read1"], e[i]["read2"], e[i]["v1"], e[i]["v2"], e[i]["ori1"], e[i]["ori2"], e[i]["pos1"] = r1, r2, v1, v2, o1, o2, p
    lay, mem = host.sr_edge_layouts(e, reads)
    got = [[(int(m["read"]), int(m["rev"]), int(m["pos"])) for m in mem[2 * i:2 * i + 2]] + [int(lay[i]["total_len"])] for i in range(4)]
    assert got == [[(0, 0, 0), (1, 0, 4), 16], [(1, 1, 0), (0, 0, 3), 13], [(0, 1, 0), (2, 0, 0), 10], [(0, 0, 0), (2, 0, 1), 10]]
    assert (lay["n_members"] == 2).all() and list(lay["first_member"]) == [0, 2, 4, 6]
    res = host.sr_consensus(reads, lay, mem, min_qual=0.5)
    assert (res.status == SR.SR_OK).all() and [int(x) for x in np.diff(res.out_off.astype(np.int64))] == [16, 13, 10, 10]
    e[1]["read2"] = 3  # a paired read: the follow-up, refused here
    with pytest.raises(HcError):
        host.sr_edge_layouts(e, reads)
