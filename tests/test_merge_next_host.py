"""hc_host_sr_merge_next (include/hcsr.h) on the CPU.  Against tests/golden/merge_next.json (the reference's calcSubreadInfo and
merge_self_overlap, run whole by make_golden_merge_next.py): the merged read's sorted clique, order among equal indexes included, and its
subread map.  Against a Python restatement of process_cliques' filters and of mergeAlongEdges' loop (src/SRBuilder.cpp:981-1001, :1260-1380),
composed over the existing mirrors of the self-overlap merge and of the next store (tests/_merge_next.py), on seeded inputs and at the edges the
loop has.  And once through a C++ program of its own, built with -fsanitize=address,undefined, on exactly sized heap blocks."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import _merge_next as M
from haploconduct_amd import consensus as SR
from haploconduct_amd import merge_next as MN
from haploconduct_amd.readstore import ReadSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDED = [(1, 0), (1, 1), (63, 0), (64, 1), (65, 64), (129, 65), (129, 64), (40, 30)]


def _golden_case():
    """every golden case as one pair of two vertices of one call: vertices 2 i (the smaller id) and 2 i + 1"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "merge_next.json")))
    cs, cq, out_off = [], [], [0]
    pair_status, first_layout, layouts, members, subreads, lay_status, pairs, singles = [], [0], [], [], [], [], [], []
    for i, c in enumerate(g["cases"]):
        m = g["mates"][c["mates"]]
        ids = sorted(set(c["v1"]))
        assert len(ids) == 2
        vertex = {ids[0]: 2 * i, ids[1]: 2 * i + 1}
        pairs.append((2 * i + 1, 2 * i) if i % 2 else (2 * i, 2 * i + 1))
        singles += [("ACGTACGTACGTACGTACGTA", "I" * 21)] * 2  # read r = vertex r
        pair_status.append(0)
        layouts.append((len(members), len(c["v1"]), 100))
        members += [(vertex[x], 0, 0, 0, (0, 0)) for x in c["v1"]]
        layouts.append((len(members), 2, 100))
        members += [(2 * i, 0, 0, 0, (0, 0)), (2 * i + 1, 0, 0, 0, (0, 0))]
        first_layout.append(first_layout[-1] + 2)
        rows = {r[0]: r[1:] for r in c["map"]}
        sub = []
        for x in ids:  # the map as calcSubreadInfo left it: the shift of :918-922 undone
            i1, s1, i2, s2 = rows[x]
            sub.append((i1, s1, i2 - c["overlap_pos"] if c["merged"] and i2 >= 0 else i2, s2))
        subreads.append(sub)
        for s, q in ((m["seq1"], m["qual1"]), (m["seq2"], m["qual2"])):
            cs.append(s)
            cq.append(q)
            out_off.append(out_off[-1] + len(s))
            lay_status.append(0)
    cons_seq, cons_qual = np.frombuffer("".join(cs).encode(), np.uint8), np.frombuffer("".join(cq).encode(), np.uint8)
    edge = M.edge_of(pair_status, first_layout, layouts, members, subreads, lay_status, out_off, cons_seq, cons_qual)
    n = 2 * len(g["cases"])
    case = M.Case(ReadSet.from_lists(singles), cons_seq, cons_qual, np.array(pairs, np.uint32), edge, np.arange(n, dtype=np.uint32), np.ones(n, np.uint8),
                  np.zeros(n, np.uint8), np.zeros(n, np.uint8))
    return g, case


def test_golden_sorted_clique_and_subread_map_after_a_self_merge():
    g, case = _golden_case()
    assert (g["min_score"], g["min_overlap"], g["min_qual"], g["mismatch"], g["min_read_len"]) == (0.99, 15, 0.99, 0.0, 0)
    got = M.call_host(case)
    n_ties = 0
    for i, c in enumerate(g["cases"]):
        ids = sorted(set(c["v1"]))
        back = {2 * i: ids[0], 2 * i + 1: ids[1]}
        assert got.overlap_pos[i] == c["overlap_pos"], i
        assert got.pair_kind[i] == (MN.MN_SINGLE_SELF if c["merged"] else MN.MN_PAIRED), i
        k = int(np.flatnonzero(got.sr_pair == i)[0])
        clique = [back[int(x)] for x in got.clique_nodes[int(got.clique_off[k]):int(got.clique_off[k + 1])]]
        assert clique == c["clique"], (i, c)
        sub = got.subreads[2 * k:2 * k + 2]
        assert sorted([back[int(s["node"])], int(s["index1"]), int(s["startpos1"]), int(s["index2"]), int(s["startpos2"])] for s in sub) == c["map"], i
        idx = [r[1] for r in c["map"]] + [r[3] for r in c["map"] if r[3] >= 0]
        n_ties += bool(c["merged"]) and len(set(idx)) < len(idx)
    assert n_ties > 50  # the order among equal indexes is what the file is for
    assert got.n_self_merged == sum(c["merged"] for c in g["cases"]) and got.n_trivials == 0 and not got.vertex_state.any()


@pytest.mark.parametrize("nv,npairs", SEEDED)
@pytest.mark.parametrize("reuse", [False, True])
def test_restatement_seeded(nv, npairs, reuse):
    c = M.make_case(1000 + nv * 7 + npairs, nv, npairs, reuse_vertex=reuse)
    for kw in M.KW_SETS:
        call, rest = M.split_kw(c, kw)
        got = M.call_host(c, **call)
        want, store = M.restatement(c, **rest)
        M.check_against_restatement(got, want, store)


def test_restatement_seeded_cases_take_every_branch():
    kinds, states, merged = set(), set(), 0
    for nv, npairs in SEEDED:
        c = M.make_case(1000 + nv * 7 + npairs, nv, npairs, reuse_vertex=True)
        call, _ = M.split_kw(c, M.KW_SETS[4])
        got = M.call_host(c, **call)
        kinds |= set(got.pair_kind.tolist())
        states |= set(got.vertex_state.tolist())
        merged += got.n_self_merged
    assert kinds == set(range(6)) and states == set(range(6)) and merged > 5  # (MN_V_BAD: test_a_vertex_whose_read_is_not_in_the_store)


def _trivials_only(singles=(), pairs=(), fwd=None, **kw):
    reads = ReadSet.from_lists(singles, pairs)
    n = reads.n_reads
    e = np.zeros(0, np.uint8)
    c = M.Case(reads, e, e, np.zeros((0, 2), np.uint32), M.empty_edge(), np.arange(n, dtype=np.uint32), np.ones(n, np.uint8) if fwd is None else np.array(fwd, np.uint8),
               np.zeros(n, np.uint8), np.zeros(n, np.uint8))
    return c


def test_restatement_n_rate_boundary_at_length_40():
    # 40 bases: 1 N is 1 < 2.0, kept; 2 N is 2 < 2.0, false (src/Read.h:226-232); 20 + 20 the same over both mates
    one, two = "N" + "A" * 39, "NN" + "A" * 38
    c = _trivials_only([(one, "I" * 40), (two, "I" * 40)], [((one[:20], "I" * 20), (one[20:], "I" * 20)), ((two[:20], "I" * 20), (two[20:], "I" * 20))])
    got = M.call_host(c)
    assert got.vertex_state.tolist() == [MN.MN_V_TRIVIAL, MN.MN_V_N_RATE, MN.MN_V_TRIVIAL, MN.MN_V_N_RATE]
    assert got.nodes["visited"].tolist() == [0, 1, 0, 1] and got.nodes["id"].tolist() == [0, 0, 1, 0]
    want, store = M.restatement(c)
    M.check_against_restatement(got, want, store)
    # the same test on a super-read (:999): a single-end one of 40 bases
    cs = np.frombuffer((one + two).encode(), np.uint8)
    cq = np.full(80, 73, np.uint8)
    reads = ReadSet.from_lists([("ACGTACGTACGTACGTACGTA", "I" * 21)] * 4)
    edge = M.edge_of([0, 0], [0, 1, 2], [(0, 2, 40), (2, 2, 40)], [(0, 0, 0, 0, (0, 0)), (1, 1, 0, 0, (0, 0)), (2, 0, 0, 0, (0, 0)), (3, 1, 0, 0, (0, 0))],
                     [[(0, 0, -1, -1), (1, 0, -1, -1)]] * 2, [0, 0], [0, 40, 80], cs, cq)
    c2 = M.Case(reads, cs, cq, np.array([(0, 1), (2, 3)], np.uint32), edge, np.arange(4, dtype=np.uint32), np.ones(4, np.uint8), np.zeros(4, np.uint8),
                np.zeros(4, np.uint8))
    got = M.call_host(c2)
    assert got.pair_kind.tolist() == [MN.MN_SINGLE, MN.MN_DROPPED_N_RATE]
    # the vertices of the dropped super-read come back as trivials with the ids behind the single
    assert got.vertex_state.tolist() == [MN.MN_V_MERGED, MN.MN_V_MERGED, MN.MN_V_TRIVIAL, MN.MN_V_TRIVIAL]
    assert got.pair_new_id.tolist() == [0, -1] and got.nodes["id"].tolist() == [0, 0, 1, 2] and got.new_read_count == 3
    M.check_against_restatement(got, *M.restatement(c2))


def test_restatement_keep_singletons_at_the_threshold():
    c = _trivials_only([("ACGTACGTAC", "I" * 10), ("ACGTACGTA", "I" * 9)], [(("ACGTA", "IIIII"), ("ACGTA", "IIIII")), (("ACGTA", "IIIII"), ("ACGT", "IIII"))])
    got = M.call_host(c, keep_singletons=10)  # get_len() < 10 (:1286): 10 stays, 9 goes; len1 + len2 for a pair
    assert got.vertex_state.tolist() == [MN.MN_V_TRIVIAL, MN.MN_V_SHORT, MN.MN_V_TRIVIAL, MN.MN_V_SHORT]
    assert got.counts["n_dropped_short"] == 2 and got.nodes["visited"].tolist() == [0, 1, 0, 1]
    M.check_against_restatement(got, *M.restatement(c, keep_singletons=10))


def test_restatement_a_short_vertex_that_is_also_an_inclusion_is_short():
    c = _trivials_only([("ACGTACGTA", "I" * 9), ("ACGTACGTAC", "I" * 10), ("NNNNNNNNNNNN", "I" * 12)])
    c.inclusions[:] = 1
    c.tip_reads[:] = 1
    got = M.call_host(c, keep_singletons=10, ignore_inclusions=True, store_tips_separately=True, inclusions=c.inclusions, tip_reads=c.tip_reads)
    assert got.vertex_state.tolist() == [MN.MN_V_SHORT, MN.MN_V_INCLUSION, MN.MN_V_N_RATE]  # :1286 before :1292 before :1298 before :1305
    assert got.tips.tolist() == [1] and got.empty and got.reads is None
    got = M.call_host(c, keep_singletons=10, ignore_inclusions=False, store_tips_separately=True, inclusions=c.inclusions, tip_reads=c.tip_reads)
    assert got.vertex_state.tolist() == [MN.MN_V_SHORT, MN.MN_V_TIP, MN.MN_V_N_RATE]
    got = M.call_host(c, keep_singletons=10, ignore_inclusions=True, store_tips_separately=True)  # both arrays NULL: nothing is an inclusion or a tip
    assert got.vertex_state.tolist() == [MN.MN_V_SHORT, MN.MN_V_TRIVIAL, MN.MN_V_N_RATE] and got.new_read_count == 1


def test_reverse_trivials_single_and_paired():
    c = _trivials_only([("AAC" + "G" * 20 + "N", "AAA" + "B" * 20 + "C")], [(("AAAC", "ABCD"), ("GGGTT", "EFGHI"))], fwd=[0, 0])
    got = M.call_host(c)
    assert M.as_lists(got.reads) == [[(b"N" + b"C" * 20 + b"GTT", b"C" + b"B" * 20 + b"AAA")], [(b"AACCC", b"IHGFE"), (b"GTTT", b"DCBA")]]  # :1342, :1355
    assert got.nodes["orientation"].tolist() == [0, 0] and got.nodes["paired"].tolist() == [0, 1] and got.nodes["len2"].tolist() == [0, 5]
    M.check_against_restatement(got, *M.restatement(c))


def test_an_empty_result():
    c = _trivials_only([("NNNN", "IIII")])
    got = M.call_host(c)
    assert got.empty and got.reads is None and got.new_read_count == 0 and got.vertex_state.tolist() == [MN.MN_V_N_RATE]
    assert got.clique_off.tolist() == [0] and got.subread_off.tolist() == [0]


def test_a_vertex_whose_read_is_not_in_the_store():
    c = _trivials_only([("ACGTACGTACGTACGTACGTA", "I" * 21)] * 2)
    c.vertex_read[1] = 7
    got = M.call_host(c)
    assert got.vertex_state.tolist() == [MN.MN_V_TRIVIAL, MN.MN_V_BAD] and got.nodes["visited"].tolist() == [0, 1] and got.counts["n_bad"] == 1


def test_fno_input_from_the_tables_and_the_length_of_tip_reads():
    from haploconduct_amd import fno

    c = M.make_case(1000 + 129 * 7 + 64, 129, 64)
    got = M.call_host(c, keep_singletons=8)
    inp = fno.input_from_merge_next(got, np.zeros(0, fno.FNO_EDGE_DTYPE), n_threads=1)
    s = inp.struct()
    assert (s.n_nodes, s.n_srs, s.new_read_count) == (129, len(got.srs), got.new_read_count)
    assert inp.clique_off.tolist() == got.clique_off.tolist() and inp.subreads.tobytes() == got.subreads.tobytes()
    text, counters = fno.find_next_overlaps(inp)  # no edges: no lines, and nothing the tables hold makes the call refuse them
    assert text == b"" and counters["n_lines"] == 0
    with pytest.raises(ValueError, match="offsets"):
        fno.Fno1Input.from_tables(got.nodes, got.srs, got.clique_off[:-1], got.clique_nodes, got.subread_off, got.subreads, np.zeros(0, fno.FNO_EDGE_DTYPE))
    with pytest.raises(ValueError, match="tip_reads"):  # the call reads a byte for every read of the store
        M.call_host(c, tip_reads=c.tip_reads[:5], store_tips_separately=True)


def test_refusals():
    import ctypes as C

    from haploconduct_amd import _native as N

    c = M.make_case(5, 8, 3)
    keep, inp, st, o, out = MN._prepare(c.pairs, c.edge, c.vertex_read, c.vertex_fwd, None, None, 0, False, False, True, 0.99, 0.99, 15, 1)
    cs = N.hc_settings()
    nb = C.c_uint64()
    off, first = np.zeros(2 * 11 + 1, np.uint64), np.zeros(12, np.uint32)

    def call():
        return N.lib.hc_host_sr_merge_next(C.byref(cs), c.reads.bases.ctypes.data, c.reads.quals.ctypes.data, c.reads.seq_off.ctypes.data,
                                           c.reads.read_first_seq.ctypes.data, c.reads.n_reads, c.cons_seq.ctypes.data, c.cons_qual.ctypes.data, c.cons_seq.size,
                                           C.byref(inp), C.byref(st), C.byref(out), None, None, 0, C.byref(nb), off.ctypes.data, first.ctypes.data)

    assert call() in (0, -1) and nb.value > 0  # the count of count-then-fetch
    fl = keep["first_layout"].copy()
    keep["first_layout"][-1] = 7  # more layouts than two a pair
    assert call() == -1
    keep["first_layout"][:] = fl
    inp.n_members = 6 * 3 + 1  # more members than hc_sr_edge_merge has room for: refused as on the device
    assert call() == -1
    inp.n_members = keep["members"].size
    inp.n_pairs, inp.n_vertices = 1 << 30, 1 << 30  # n_pairs + n_vertices = 2^31: refused before anything is read
    assert call() == -1
    with pytest.raises(ValueError):
        M.call_host(M.Case(c.reads, c.cons_seq, c.cons_qual, c.pairs, c.edge, c.vertex_read, c.vertex_fwd[:3], None, None))


PROGRAM = r'''
// Reads the cases the test wrote (sizes, then the arrays as they lie in memory), runs hc_host_sr_merge_next on heap blocks of exactly the
// sizes the contract names (count, then fetch) and prints what came back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "hcsr.h"
namespace hc { int set_last_error(int s, const std::string&) { return s; } }
template <typename T> static T* blk(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
    return p;
}
template <typename T> static T* room(size_t n) { return (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1); }
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[12];
    int n_cases = 0;
    while (fread(h, 8, 12, f) == 12) {
        const uint64_t np = h[0], nl = h[1], nm = h[2], nv = h[3], n_reads = h[4], n_seq = h[5], n_store = h[6], n_cons = h[7];
        hc_sr_merge_next_settings st;
        memset(&st, 0, sizeof st);
        st.keep_singletons = (uint32_t)h[8];
        st.ignore_inclusions = (uint32_t)h[9];
        st.store_tips_separately = (uint32_t)h[10];
        st.self.min_score = 0.99, st.self.min_qual = 0.99, st.self.min_overlap = 15, st.self.n_threads = 1;
        const bool with_arrays = h[11] != 0;
        hc_sr_merge_next_input in;
        memset(&in, 0, sizeof in);
        in.n_pairs = np, in.n_members = nm, in.n_vertices = nv;
        in.pairs = blk<uint32_t>(f, 2 * np);
        in.pair_status = blk<uint32_t>(f, np);
        in.first_layout = blk<uint64_t>(f, np + 1);
        in.layouts = blk<hc_sr_layout>(f, nl);
        in.members = blk<hc_sr_member>(f, nm);
        in.status = blk<uint32_t>(f, nl);
        in.out_off = blk<uint64_t>(f, nl + 1);
        in.subreads = blk<hc_sr_subread_info>(f, 2 * np);
        in.vertex_read = blk<uint32_t>(f, nv);
        in.vertex_fwd = blk<uint8_t>(f, nv);
        uint8_t* incl = blk<uint8_t>(f, nv);
        uint8_t* tips = blk<uint8_t>(f, n_reads);
        in.inclusions = with_arrays ? incl : NULL;
        in.tip_reads = with_arrays ? tips : NULL;
        uint8_t *bases = blk<uint8_t>(f, n_store), *quals = blk<uint8_t>(f, n_store);
        uint64_t* seq_off = blk<uint64_t>(f, n_seq + 1);
        uint32_t* first = blk<uint32_t>(f, n_reads + 1);
        uint8_t *cs = blk<uint8_t>(f, n_cons), *cq = blk<uint8_t>(f, n_cons);
        hc_sr_merge_next_output o;
        memset(&o, 0, sizeof o);
        o.pair_kind = room<uint32_t>(np), o.pair_new_id = room<int32_t>(np), o.overlap_pos = room<int32_t>(np), o.self_score = room<double>(np);
        o.vertex_state = room<uint32_t>(nv), o.nodes = room<hc_fno_read>(nv), o.srs = room<hc_fno_read>(np), o.sr_pair = room<uint32_t>(np);
        o.clique_off = room<uint64_t>(np + 1), o.clique_nodes = room<uint64_t>(4 * np), o.subread_off = room<uint64_t>(np + 1);
        o.subreads = room<hc_fno_subread>(2 * np), o.tips = room<uint32_t>(nv);
        uint64_t* out_off = room<uint64_t>(2 * (np + nv) + 1);
        uint32_t* out_first = room<uint32_t>(np + nv + 1);
        hc_settings ec;
        memset(&ec, 0, sizeof ec);
        uint64_t nb = 0;
        int rc = hc_host_sr_merge_next(&ec, bases, quals, seq_off, first, (uint32_t)n_reads, cs, cq, n_cons, &in, &st, &o, NULL, NULL, 0, &nb, out_off, out_first);
        uint8_t *ob = room<uint8_t>(nb), *oq = room<uint8_t>(nb);
        if (rc != HC_SR_NEXT_EMPTY) rc = hc_host_sr_merge_next(&ec, bases, quals, seq_off, first, (uint32_t)n_reads, cs, cq, n_cons, &in, &st, &o, ob, oq, nb, &nb, out_off, out_first);
        unsigned long long sum = 0;
        for (uint64_t i = 0; i < nb; i++) sum = sum * 131 + ob[i] + 7 * oq[i];
        for (uint64_t i = 0; i < o.clique_off[o.n_srs]; i++) sum = sum * 131 + o.clique_nodes[i];
        printf("%d %llu %llu %llu %llu %llu %llu %llu %llu\n", rc, (unsigned long long)o.n_singles, (unsigned long long)o.n_trivials, (unsigned long long)o.n_paired,
               (unsigned long long)o.n_tips, (unsigned long long)o.n_self_merged, (unsigned long long)o.new_read_count, (unsigned long long)nb, sum);
        for (const void* p : {(const void*)in.pairs, (const void*)in.pair_status, (const void*)in.first_layout, (const void*)in.layouts, (const void*)in.members,
                              (const void*)in.status, (const void*)in.out_off, (const void*)in.subreads, (const void*)in.vertex_read, (const void*)in.vertex_fwd,
                              (const void*)incl, (const void*)tips, (const void*)bases, (const void*)quals, (const void*)seq_off, (const void*)first, (const void*)cs,
                              (const void*)cq, (const void*)o.pair_kind, (const void*)o.pair_new_id, (const void*)o.overlap_pos, (const void*)o.self_score,
                              (const void*)o.vertex_state, (const void*)o.nodes, (const void*)o.srs, (const void*)o.sr_pair, (const void*)o.clique_off,
                              (const void*)o.clique_nodes, (const void*)o.subread_off, (const void*)o.subreads, (const void*)o.tips, (const void*)out_off,
                              (const void*)out_first, (const void*)ob, (const void*)oq})
            free((void*)p);
        n_cases++;
    }
    fclose(f);
    printf("%d cases\n", n_cases);
    return 0;
}
'''


def _blob(c, keep_singletons, ignore_inclusions, store_tips, with_arrays):
    e = c.edge
    nl = int(e.first_layout[-1])
    arrays = [c.pairs.astype(np.uint32), e.pair_status.astype(np.uint32), e.first_layout.astype(np.uint64), e.layouts[:nl], e.members, e.result.status[:nl].astype(np.uint32),
              e.result.out_off[:nl + 1].astype(np.uint64), e.subreads, c.vertex_read, c.vertex_fwd, c.inclusions, c.tip_reads, c.reads.bases, c.reads.quals, c.reads.seq_off,
              c.reads.read_first_seq, c.cons_seq, c.cons_qual]
    head = struct.pack("<12Q", len(c.pairs), nl, len(e.members), len(c.vertex_read), c.reads.n_reads, c.reads.n_seq, c.reads.bases.size, c.cons_seq.size, keep_singletons,
                       ignore_inclusions, store_tips, with_arrays)
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _sum(res):
    s = 0
    if res.reads is not None:
        for b, q in zip(res.reads.bases.tolist(), res.reads.quals.tolist()):
            s = (s * 131 + b + 7 * q) & (2 ** 64 - 1)
    for x in res.clique_nodes.tolist():
        s = (s * 131 + x) & (2 ** 64 - 1)
    return s


def test_mirror_under_asan_ubsan(tmp_path):
    """the mirror's host sources and a program with its own main, no Python and no device in the process"""
    blobs, want = [], []
    for nv, npairs in SEEDED:
        c = M.make_case(1000 + nv * 7 + npairs, nv, npairs, reuse_vertex=True)
        for ks, ii, ts, wa in ((0, 0, 0, 0), (9, 1, 1, 1)):
            blobs.append(_blob(c, ks, ii, ts, wa))
            r = M.call_host(c, keep_singletons=ks, ignore_inclusions=ii, store_tips_separately=ts, inclusions=c.inclusions if wa else None,
                            tip_reads=c.tip_reads if wa else None)
            want.append("%d %d %d %d %d %d %d %d %d" % (1 if r.empty else 0, r.n_singles, r.n_trivials, r.n_paired, len(r.tips), r.n_self_merged, r.new_read_count,
                                                        0 if r.reads is None else r.reads.bases.size, _sum(r)))
    data = tmp_path / "cases.bin"
    data.write_bytes(b"".join(blobs))
    src = tmp_path / "merge_next_asan_main.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "merge_next_asan")
    host = os.path.join(ROOT, "haploconduct_amd", "csrc", "host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # the mirrors include the headers they share with the kernels
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(["g++", "-std=c++17", *san, "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), "-o", exe,
                        str(src), os.path.join(host, "SrMergeNext.cpp"), os.path.join(host, "SrNextReads.cpp"), os.path.join(host, "SrSelfOverlap.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(data)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"), capture_output=True, text=True, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and lines[-1] == f"{len(blobs)} cases", (r.stdout[-1000:], r.stderr[-3000:])
    assert lines[:-1] == want
