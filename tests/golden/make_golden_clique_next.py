#!/usr/bin/env python3
"""Generates tests/golden/clique_next.json: (a) what SRBuilder::merge_self_overlap leaves of the sorted clique and subread map of a paired
super-read of 3 - 40 vertices, (b) what the gate of SRBuilder::cliquesToSuperreads (src/SRBuilder.cpp:1056-1084) selects from a clique file.

Runs only in the build container (needs /root/reference).  Both probes are compiled in a temporary directory from line ranges streamed
from the reference and are never stored.

(a) is make_golden_merge_next.py's probe_merge_next as it is (calcSubreadInfo, then merge_self_overlap whole): it takes lists of any
length.  A case is a clique of n paired vertices — both layouts list every vertex once, in orders of their own, with ascending
positions that repeat — and a pair of mates.  Stored: the inputs, whether the pair merged, overlap_pos, the merged read's
get_sorted_clique(0) in list order and its subread map.  For more than two vertices the order among equal indexes in that list is the
unordered_map's iteration order followed by libstdc++'s std::sort (unstable beyond 16 elements): the tests compare it as a sequence of
index groups and, inside a group, as a multiset of vertices.

(b) is the loop of :1056-1084 with its own statements: the probe opens the file, declares what the lines before :1056 declare (a
std::vector<bool> in place of boost::dynamic_bitset<>: the loop only indexes it), streams :1056-1084 and closes the loop with a brace of
its own, since the loop's own brace lies behind the batching of :1102-1106.

    python tests/golden/make_golden_clique_next.py
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_merge_next import build_probe  # noqa: E402
from make_golden_self_overlap import REF, ROOT, quiet  # noqa: E402

SELECT_HEAD = r"""
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "Types.h"
extern "C" int probe_select(const char* path, int remove_multi_occ, unsigned int min_clique_size, unsigned int n_vertices, unsigned int* out_nodes,
                            unsigned long* out_off, int* n_singletons) {
    struct { bool remove_multi_occ; } program_settings = {remove_multi_occ != 0};
    unsigned int minCliqueSize = min_clique_size;
    unsigned long clique_count = 0;
    int singleton_count = 0;
    std::ifstream cliquefile(path);
    std::string cliqueline;
    std::vector< std::vector< node_id_t> > SR_clique_vec;
    node_id_t totalcount = 0;
    std::vector<bool> used_nodes(n_vertices);
"""
SELECT_TAIL = r"""
    }  // (the probe's own: the loop's brace lies behind :1102-1106)
    unsigned long n = 0;
    out_off[0] = 0;
    for (unsigned long i = 0; i < SR_clique_vec.size(); i++) {
        for (auto x : SR_clique_vec[i]) out_nodes[n++] = x;
        out_off[i + 1] = n;
    }
    *n_singletons = singleton_count;
    (void)totalcount;
    (void)clique_count;
    return (int)SR_clique_vec.size();
}
"""


def build_select_probe(tmp):
    src = os.path.join(tmp, "select.cpp")
    sr = open(os.path.join(REF, "SRBuilder.cpp")).read().split("\n")
    with open(src, "w") as f:
        f.write(SELECT_HEAD)
        f.write("\n".join(sr[1055:1084]) + "\n")
        f.write(SELECT_TAIL)
    so = os.path.join(tmp, "select.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-I", REF, "-o", so, src], check=True)
    return C.CDLL(so)


def run_merge(dll, c, mates):
    s1, q1, s2, q2 = mates[c["mates"]]
    n = len(c["v1"])
    ai = lambda x: (C.c_int * max(1, len(x)))(*x)
    au = lambda x: (C.c_uint * max(1, len(x)))(*x)
    out_len, n_clique, n_map = C.c_int(), C.c_int(), C.c_int()
    clique, nodes, info = (C.c_uint * (2 * n))(), (C.c_uint * n)(), (C.c_int * (4 * n))()
    r = dll.probe_merge_next(ai(c["pos1"]), au(c["v1"]), n, ai(c["pos2"]), au(c["v2"]), n, c["trim1"], c["trim2"], s1.encode(), q1.encode(), s2.encode(),
                             q2.encode(), C.byref(out_len), clique, C.byref(n_clique), nodes, info, C.byref(n_map))
    assert r in (0, 1) and n_map.value == n and n_clique.value <= 2 * n
    c["merged"] = r
    c["overlap_pos"] = out_len.value - len(s2) if r else -1
    c["clique"] = [int(clique[i]) for i in range(n_clique.value)]
    c["map"] = sorted([int(nodes[i])] + [int(info[4 * i + k]) for k in range(4)] for i in range(n))


def indexes(c):
    return [r[1] for r in c["map"]] + [r[3] for r in c["map"] if r[3] >= 0]


def merge_cases(rng):
    genome = "".join(rng.choice("ACGT") for _ in range(4000))
    mates, want = [], []
    for a, l1, p, l2 in ((100, 60, 40, 50), (300, 90, 20, 100), (600, 40, 7, 45)):
        mates.append((genome[a:a + l1], "I" * l1, genome[a + p:a + p + l2], "I" * l2))
        want.append(p)
    mates.append((genome[1000:1060], "I" * 60, genome[2000:2050], "I" * 50))
    want.append(-1)
    cases = []
    sizes = [3, 4, 5, 7, 8, 9, 12, 16, 17, 23, 31, 32, 33, 40]
    for mi, p in enumerate(want):
        shift = p if p > 0 else 11
        for n in sizes:
            for style in range(2):
                # vertex ids: small and dense, or spread so that the map's buckets differ
                ids = rng.sample(range(3 * n), n) if style == 0 else rng.sample(range(10 ** 6), n - 1) + [4000000000 + n]
                v1, v2 = ids[:], ids[:]
                rng.shuffle(v1)
                rng.shuffle(v2)

                def positions():
                    step = [0] + [rng.choice((0, 0, 1, 3, shift)) for _ in range(n - 1)]  # ascending, with repeats
                    out, at = [], 0
                    for s in step:
                        at += s
                        out.append(at)
                    return out

                cases.append(dict(mates=mi, v1=v1, pos1=positions(), v2=v2, pos2=positions(), trim1=rng.choice((0, 3)), trim2=rng.choice((0, 3, shift))))
    return mates, want, cases


def select_files(rng):
    """clique files as lists of lines (a line: vertex ids; a comment line gives no vertex, :1061)"""
    files = []
    for k in range(44):
        nv = rng.choice((6, 12, 30, 64))
        lines = []
        for _ in range(rng.randrange(1, 14)):
            style = rng.random()
            if style < 0.1:
                lines.append("# cliques of round %d" % k)
            elif style < 0.25:
                lines.append(str(rng.randrange(nv)))
            else:
                lines.append(" ".join(str(x) for x in rng.sample(range(nv), rng.randrange(2, min(nv, 9)))))
        files.append(dict(n_vertices=nv, min_clique_size=rng.choice((2, 2, 3, 4)), lines=lines))
    # by hand: a filter leaves a singleton; a filter leaves a clique below minCliqueSize; a filter empties a clique; a clique the gate
    # rejected does not use its vertices
    files.append(dict(n_vertices=8, min_clique_size=2, lines=["0 1 2", "2 3", "3 4 5"]))
    files.append(dict(n_vertices=8, min_clique_size=3, lines=["0 1 2", "1 2 3 4", "3 4 5", "5 6"]))
    files.append(dict(n_vertices=8, min_clique_size=2, lines=["0 1", "1 0", "2", "0 1 2 3"]))
    files.append(dict(n_vertices=8, min_clique_size=3, lines=["0 1", "0 1 2", "1 3 4"]))
    return files


def run_select(dll, tmp, f, remove_multi_occ):
    path = os.path.join(tmp, "cliques.txt")
    with open(path, "w") as fh:
        fh.write("".join(line + "\n" for line in f["lines"]))
    n_items = sum(len(line.split()) for line in f["lines"]) + 1
    nodes, off, n1 = (C.c_uint * n_items)(), (C.c_ulong * (len(f["lines"]) + 1))(), C.c_int()
    k = dll.probe_select(path.encode(), remove_multi_occ, f["min_clique_size"], f["n_vertices"], nodes, off, C.byref(n1))
    return dict(cliques=[[int(nodes[j]) for j in range(off[i], off[i + 1])] for i in range(k)], n_singletons=n1.value)


def main():
    rng = random.Random(20241020)
    mates, want, cases = merge_cases(rng)
    files = select_files(rng)
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        with quiet():
            for c in cases:
                run_merge(dll, c, mates)
        sel = build_select_probe(tmp)
        for f in files:
            f["plain"] = run_select(sel, tmp, f, 0)
            f["remove_multi_occ"] = run_select(sel, tmp, f, 1)
    for c in cases:
        assert c["overlap_pos"] == want[c["mates"]], (c, want)
    merged = [c for c in cases if c["merged"]]
    n_ties = sum(len(set(indexes(c))) < len(indexes(c)) for c in merged)
    n_long = sum(len(c["clique"]) > 16 for c in merged)
    assert len(merged) >= 60 and n_ties >= 20 and n_long >= 20, (len(merged), n_ties, n_long)
    assert any(f["remove_multi_occ"]["n_singletons"] > f["plain"]["n_singletons"] for f in files)
    out = dict(provenance="probe with substitutes: (a) src/SRBuilder.cpp:536-595, :872-955 and :289-535, src/EdgeCalculator.cpp:26-139 with the genuine "
                          "Read.h / Types.h in declaration shells for SRBuilder and EdgeCalculator, boost::dynamic_bitset replaced by a stand-in; "
                          "(b) src/SRBuilder.cpp:1056-1084 with the declarations in front of it restated, std::vector<bool> for the bitset and a "
                          "closing brace of the probe's own",
               min_score=0.99, min_overlap=15, mismatch=0.0, min_read_len=0, min_qual=0.99,
               mates=[dict(seq1=m[0], qual1=m[1], seq2=m[2], qual2=m[3]) for m in mates], cases=cases, select=files)
    path = os.path.join(ROOT, "tests", "golden", "clique_next.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(f"{len(cases)} cases, {len(merged)} merged, {n_ties} with equal indexes, {n_long} with more than 16 entries; {len(files)} clique files; "
          f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
