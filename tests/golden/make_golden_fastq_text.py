#!/usr/bin/env python3
"""Generates tests/golden/fastq_text.json: the bytes SRBuilder's four FASTQ writers leave in singles.fastq, paired1.fastq, paired2.fastq
and removed_tip_sequences.fastq for a dozen small read sets.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory, in the manner of
make_golden_merge_next.py: src/SRBuilder.cpp:1386-1556 (writeTipsToFile, writeTrivialsToFile, writeSinglesToFile, writePairsToFile, whole)
streamed from the reference by line range and never stored, the genuine Read.h and Types.h included from the reference tree, and a
declaration-only shell for SRBuilder that holds PATH, tips_vec, trivial_SR_vec and the four declarations.  Nothing is substituted beyond
the shell ("probe with substitutes: none beyond the shell").  PATH is a temporary directory.

A case is a list of reads, each with the vector it sat in when the writers ran: "singles" (single_SR_vec), "trivials" (trivial_SR_vec, single-end
and paired mixed, in vertex order), "pairs" (paired_SR_vec), "tips" (tips_vec).  The probe runs the writers in the order mergeAlongEdges
calls them (:1280, :1377-1379): writeSinglesToFile from count = 0, the trivials numbered on from there as :1370-1371 numbers them,
writeTrivialsToFile, writePairsToFile, writeTipsToFile.  Stored: the reads and the bytes of the four files.  subreads.txt, which the same
writers append to, is not recorded: its order is the hash table's, and tests/golden/originals.json covers it.

    python tests/golden/make_golden_fastq_text.py
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_self_overlap import REF, ROOT  # noqa: E402

SHELL_HEAD = r"""
#include <assert.h>
#include <algorithm>
#include <deque>
#include <fstream>
#include <iostream>
#include <list>
#include <string>
#include <unordered_map>
#include <vector>
#include "Read.h"
#include "Types.h"
class SRBuilder {
public:
    std::string PATH;
    std::deque<Read> tips_vec;
    std::deque<Read> trivial_SR_vec;
    void writeTipsToFile();
    void writeTrivialsToFile();
    void writeSinglesToFile(std::deque<Read>& singles, read_id_t& count);
    void writePairsToFile(std::deque<Read>& pairs, read_id_t& count);
};
"""

SHELL_TAIL = r"""
// vec: 0 = single_SR_vec, 1 = trivial_SR_vec, 2 = paired_SR_vec, 3 = tips_vec; reads of one vector in the order given
extern "C" long probe_fastq(const char* path, int n, const int* vec, const int* paired, const char** s1, const char** q1, const char** s2,
                            const char** q2) {
    SRBuilder b;
    b.PATH = path;
    std::deque<Read> singles, pairs;
    read_id_t count = 0;
    for (int i = 0; i < n; i++)
        if (vec[i] == 0) singles.push_back(Read(false, true, 0, s1[i], "", q1[i], ""));
    b.writeSinglesToFile(singles, count);  // :1279-1280
    for (int i = 0; i < n; i++)
        if (vec[i] == 1) b.trivial_SR_vec.push_back(Read(paired[i] != 0, true, count++, s1[i], s2[i], q1[i], q2[i]));  // :1370-1371
    for (int i = 0; i < n; i++)
        if (vec[i] == 2) pairs.push_back(Read(true, true, 0, s1[i], s2[i], q1[i], q2[i]));
    for (int i = 0; i < n; i++)
        if (vec[i] == 3) b.tips_vec.push_back(Read(paired[i] != 0, false, 1000 + i, s1[i], s2[i], q1[i], q2[i]));
    b.writeTrivialsToFile();  // :1377
    b.writePairsToFile(pairs, count);  // :1378
    b.writeTipsToFile();  // :1379
    return (long)count;
}
"""

VECS = ("singles", "trivials", "pairs", "tips")
FILES = ("singles.fastq", "paired1.fastq", "paired2.fastq", "removed_tip_sequences.fastq")


def build_probe(tmp):
    src = os.path.join(tmp, "probe.cpp")
    sr = open(os.path.join(REF, "SRBuilder.cpp")).read().split("\n")
    with open(src, "w") as f:
        f.write(SHELL_HEAD)
        f.write("\n".join(sr[1385:1556]) + "\n")
        f.write(SHELL_TAIL)
    so = os.path.join(tmp, "probe.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-I", REF, "-o", so, src], check=True)
    dll = C.CDLL(so)
    dll.probe_fastq.restype = C.c_long
    return dll


def run(dll, case, tmp, k):
    out = os.path.join(tmp, f"case{k}") + os.sep
    os.mkdir(out)
    reads = case["reads"]
    n = len(reads)
    strs = lambda key: (C.c_char_p * max(1, n))(*[r.get(key, "").encode() for r in reads])
    case["new_read_count"] = int(dll.probe_fastq(out.encode(), n, (C.c_int * max(1, n))(*[VECS.index(r["vec"]) for r in reads]),
                                                 (C.c_int * max(1, n))(*[int("seq2" in r) for r in reads]), strs("seq1"), strs("qual1"), strs("seq2"),
                                                 strs("qual2")))
    case["files"] = {}
    for name in FILES:  # a file the writers never opened is an empty contribution
        path = os.path.join(out, name)
        case["files"][name] = open(path, "rb").read().decode("ascii") if os.path.exists(path) else ""


def main():
    rng = random.Random(20261020)
    quals = "".join(chr(c) for c in range(33, 127))

    def read(vec, paired, lo=1, hi=70):
        r = dict(vec=vec)
        for m in ("1", "2") if paired else ("1",):
            n = rng.randint(lo, hi)
            r["seq" + m] = "".join(rng.choice("ACGTN") for _ in range(n))
            r["qual" + m] = "".join(rng.choice(quals) for _ in range(n))
        return r

    def case(name, n_singles=0, n_triv_s=0, n_triv_p=0, n_pairs=0, n_tip_s=0, n_tip_p=0, **kw):
        triv = [read("trivials", False, **kw) for _ in range(n_triv_s)] + [read("trivials", True, **kw) for _ in range(n_triv_p)]
        tips = [read("tips", False, **kw) for _ in range(n_tip_s)] + [read("tips", True, **kw) for _ in range(n_tip_p)]
        rng.shuffle(triv)
        rng.shuffle(tips)
        reads = [read("singles", False, **kw) for _ in range(n_singles)] + triv + [read("pairs", True, **kw) for _ in range(n_pairs)] + tips
        rng.shuffle(reads)  # (the probe takes each vector's reads in the order they appear)
        return dict(name=name, reads=reads)

    cases = [
        case("single-end only", n_singles=5),
        case("paired only", n_pairs=4),
        case("one single-end read of one base", n_singles=1, lo=1, hi=1),
        case("trivials only, mixed", n_triv_s=3, n_triv_p=3),
        case("mixed with trivials", n_singles=3, n_triv_s=2, n_triv_p=2, n_pairs=3),
        case("mixed with tips of both kinds", n_singles=2, n_triv_s=2, n_triv_p=1, n_pairs=2, n_tip_s=3, n_tip_p=3),
        case("tips only paired", n_singles=1, n_tip_p=2),
        case("tips only single-end", n_pairs=1, n_tip_s=2),
        case("no tips", n_singles=2, n_triv_p=2, n_pairs=2),
        case("ids cross 9 -> 10", n_singles=4, n_triv_s=3, n_triv_p=3, n_pairs=3, n_tip_s=6, n_tip_p=6, hi=12),
        case("ids cross 99 -> 100", n_singles=40, n_triv_s=25, n_triv_p=25, n_pairs=22, n_tip_s=51, n_tip_p=52, hi=6),
        case("nothing", 0),
    ]
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        for k, c in enumerate(cases):
            run(dll, c, tmp, k)
    for c in cases:
        by = {v: [r for r in c["reads"] if r["vec"] == v] for v in VECS}
        assert c["new_read_count"] == len(by["singles"]) + len(by["trivials"]) + len(by["pairs"]), c["name"]
        f = c["files"]
        assert f["singles.fastq"].count("\n") == 4 * (len(by["singles"]) + sum("seq2" not in r for r in by["trivials"])), c["name"]
        assert f["paired1.fastq"].count("\n") == f["paired2.fastq"].count("\n") == 4 * (len(by["pairs"]) + sum("seq2" in r for r in by["trivials"]))
        assert f["removed_tip_sequences.fastq"].count("\n") == 4 * sum(2 if "seq2" in r else 1 for r in by["tips"]), c["name"]
    out = dict(provenance="probe with substitutes: none beyond the shell — src/SRBuilder.cpp:1386-1556 with the genuine Read.h / Types.h in a "
                          "declaration-only SRBuilder holding PATH, tips_vec, trivial_SR_vec and the four writers' declarations; the writers run in "
                          "mergeAlongEdges' order (:1280, :1377-1379)",
               cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "fastq_text.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(f"{len(cases)} cases, {sum(len(c['reads']) for c in cases)} reads, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
