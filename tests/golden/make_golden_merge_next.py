#!/usr/bin/env python3
"""Generates tests/golden/merge_next.json: what SRBuilder::merge_self_overlap leaves of a super-read's sorted clique and subread map.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory, in the manner of
make_golden_self_overlap.py: src/SRBuilder.cpp:536-595 (calcSubreadInfo), :872-955 (merge_self_overlap, whole) and :289-535
(phred_to_prob, consensus_pos, consensus) and src/EdgeCalculator.cpp:26-139 streamed from the reference by line range and never stored,
the genuine Read.h and Types.h included from the reference tree, declaration-only shells for SRBuilder and EdgeCalculator and the
few-line stand-in for boost::dynamic_bitset.  The vectors are therefore "probe with substitutes".

A case is calcSubreadInfo's input for a clique of two vertices (the two position lists, the two vertex lists, the two trim positions)
and a pair of mates; the probe runs calcSubreadInfo, puts the map into a paired Read with those mates and runs merge_self_overlap.
Stored: the inputs, whether the pair merged, overlap_pos, the merged read's get_sorted_clique(0) in list order and its subread map.
The order among equal indexes in that clique is the thing pinned: it comes from the unordered_map's iteration order followed by
libstdc++'s std::sort on at most four elements.

What the loop of src/SRBuilder.cpp:1260-1373 does cannot be probed without supplying the behaviour of OverlapGraph and FastqStorage;
tests/test_merge_next_host.py pins it by a Python restatement that cites the lines.

    python tests/golden/make_golden_merge_next.py
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_self_overlap import REF, ROOT, SHELL_HEAD, quiet  # noqa: E402

SHELL_HEAD_MN = SHELL_HEAD.replace(
    "    Read merge_self_overlap(Read superread, EdgeCalculator & edge_calculator);",
    "    Read merge_self_overlap(Read superread, EdgeCalculator & edge_calculator);\n"
    "    std::unordered_map< node_id_t, SubreadInfo > calcSubreadInfo(int trim_pos1, int trim_pos2, std::list<int> pos_list1, std::list<int> pos_list2,\n"
    "                                                                  std::list<node_id_t> sorted_vertices1, std::list<node_id_t> sorted_vertices2);")
assert SHELL_HEAD_MN != SHELL_HEAD

SHELL_TAIL = r"""
extern "C" int probe_merge_next(const int* pos1, const unsigned int* v1, int n1, const int* pos2, const unsigned int* v2, int n2, int trim1, int trim2,
                                const char* s1, const char* q1, const char* s2, const char* q2, int* out_len, unsigned int* clique, int* n_clique,
                                unsigned int* map_nodes, int* map_info, int* n_map) {
    SRBuilder b;
    b.minQual = 0.99;
    b.program_settings.min_clique_size = 2;
    EdgeCalculator ec;
    ec.program_settings.mismatch = 0.0;
    ec.program_settings.min_read_len = 0;
    std::list<int> p1(pos1, pos1 + n1), p2(pos2, pos2 + n2);
    std::list<node_id_t> l1(v1, v1 + n1), l2(v2, v2 + n2);
    std::unordered_map< node_id_t, SubreadInfo > m = b.calcSubreadInfo(trim1, trim2, p1, p2, l1, l2);
    Read r(true, true, 7, s1, s2, q1, q2);
    r.set_sorted_clique(1, l1);
    r.set_sorted_clique(2, l2);
    r.set_subread_map(m);
    Read out = b.merge_self_overlap(r, ec);
    const bool merged = !out.is_paired();
    *out_len = merged ? (int)out.get_seq(0).size() : -1;
    std::list<node_id_t> c = out.get_sorted_clique(merged ? 0 : 1);
    *n_clique = 0;
    for (auto x : c) clique[(*n_clique)++] = x;
    std::unordered_map< node_id_t, SubreadInfo > om = out.get_subreadMap();
    *n_map = 0;
    for (auto it : om) {
        map_nodes[*n_map] = it.first;
        map_info[4 * *n_map] = it.second.index1;
        map_info[4 * *n_map + 1] = it.second.startpos1;
        map_info[4 * *n_map + 2] = it.second.index2;
        map_info[4 * *n_map + 3] = it.second.startpos2;
        (*n_map)++;
    }
    return merged ? 1 : 0;
}
"""


def build_probe(tmp):
    src = os.path.join(tmp, "probe.cpp")
    sr = open(os.path.join(REF, "SRBuilder.cpp")).read().split("\n")
    ec = open(os.path.join(REF, "EdgeCalculator.cpp")).read().split("\n")
    with open(src, "w") as f:
        f.write(SHELL_HEAD_MN)
        f.write("\n".join(ec[25:139]) + "\n")
        f.write("\n".join(sr[288:535]) + "\n")
        f.write("\n".join(sr[535:595]) + "\n")
        f.write("\n".join(sr[871:955]) + "\n")
        f.write(SHELL_TAIL)
    so = os.path.join(tmp, "probe.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-I", REF, "-o", so, src], check=True)
    return C.CDLL(so)


def run(dll, c, mates):
    s1, q1, s2, q2 = mates[c["mates"]]
    ai = lambda x: (C.c_int * max(1, len(x)))(*x)
    au = lambda x: (C.c_uint * max(1, len(x)))(*x)
    out_len, n_clique, n_map = C.c_int(), C.c_int(), C.c_int()
    clique, nodes, info = (C.c_uint * 16)(), (C.c_uint * 8)(), (C.c_int * 32)()
    r = dll.probe_merge_next(ai(c["pos1"]), au(c["v1"]), len(c["v1"]), ai(c["pos2"]), au(c["v2"]), len(c["v2"]), c["trim1"], c["trim2"], s1.encode(),
                             q1.encode(), s2.encode(), q2.encode(), C.byref(out_len), clique, C.byref(n_clique), nodes, info, C.byref(n_map))
    assert r in (0, 1)
    c["merged"] = r
    c["overlap_pos"] = out_len.value - len(s2) if r else -1
    c["clique"] = [int(clique[i]) for i in range(n_clique.value)]
    c["map"] = sorted([int(nodes[i])] + [int(info[4 * i + k]) for k in range(4)] for i in range(n_map.value))


def main():
    rng = random.Random(20241019)
    genome = "".join(rng.choice("ACGT") for _ in range(4000))
    # the mates: three that merge at a known offset, one that does not
    mates, want = [], []
    for a, l1, p, l2 in ((100, 60, 40, 50), (300, 90, 20, 100), (600, 40, 7, 45)):
        mates.append((genome[a:a + l1], "I" * l1, genome[a + p:a + p + l2], "I" * l2))
        want.append(p)
    mates.append((genome[1000:1060], "I" * 60, genome[2000:2050], "I" * 50))
    want.append(-1)
    id_pairs = [(0, 1), (1, 0), (3, 16), (16, 3), (5, 18), (12, 13), (100000, 7), (7, 100000), (4000000000, 26), (26, 39), (1000, 2013), (2, 9)]
    cases = []
    for mi, p in enumerate(want):
        shift = p if p > 0 else 11
        values = [0, 3, shift, shift + 3, 2 * shift]
        for a, b in id_pairs:
            # paired super-reads: both vertices in both layouts, either order (:692-693)
            for k in range(4):
                v1 = [a, b] if k & 1 else [b, a]
                v2 = [a, b] if k & 2 else [b, a]
                pos1 = [0, rng.choice(values)]
                pos2 = [0, rng.choice(values)]
                cases.append(dict(mates=mi, v1=v1, pos1=pos1, v2=v2, pos2=pos2, trim1=rng.choice((0, 3)), trim2=rng.choice((0, 3, shift))))
            # single-end shapes (trim_pos2 = -1): index2 < 0 for a single-end member, a paired member listed twice (:544-556)
            for v1 in ([a, b], [a, b, b], [b, a, b], [b, b, a], [a, a, b, b], [a, b, a, b]):
                pos1 = sorted([0] + [rng.choice(values) for _ in v1[1:]])
                cases.append(dict(mates=mi, v1=v1, pos1=pos1, v2=[], pos2=[], trim1=rng.choice((0, 3, shift)), trim2=-1))
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        with quiet():
            for c in cases:
                run(dll, c, mates)
    for c in cases:
        assert c["overlap_pos"] == want[c["mates"]], (c, want)
    n_ties = sum(len(set(_indexes(c))) < len(_indexes(c)) for c in cases if c["merged"])
    assert n_ties > 50, n_ties
    out = dict(provenance="probe with substitutes: src/SRBuilder.cpp:536-595, :872-955 and :289-535, src/EdgeCalculator.cpp:26-139 with the genuine "
                          "Read.h / Types.h in declaration shells for SRBuilder and EdgeCalculator, boost::dynamic_bitset replaced by a stand-in",
               min_score=0.99, min_overlap=15, mismatch=0.0, min_read_len=0, min_qual=0.99,
               mates=[dict(seq1=m[0], qual1=m[1], seq2=m[2], qual2=m[3]) for m in mates], cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "merge_next.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(f"{len(cases)} cases, {sum(c['merged'] for c in cases)} merged, {n_ties} with equal indexes, {os.path.getsize(path)} bytes -> {path}")


def _indexes(c):
    out = []
    for row in c["map"]:
        out.append(row[1])
        if row[3] >= 0:
            out.append(row[3])
    return out


if __name__ == "__main__":
    main()
