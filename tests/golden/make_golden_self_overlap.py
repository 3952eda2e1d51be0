#!/usr/bin/env python3
"""Generates tests/golden/self_overlap.json with the reference's own SRBuilder::merge_self_overlap, run whole.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory:
src/SRBuilder.cpp:872-955 (merge_self_overlap) and :289-535 (phred_to_prob, consensus_pos, consensus) and
src/EdgeCalculator.cpp:26-139 (score, phred_to_prob, overlap_score) streamed from the reference by line range, the genuine
Read.h and Types.h (both Boost-free) included from the reference tree, and build-owned declaration shells (below) for
SRBuilder and EdgeCalculator with the members that text uses, plus the few-line stand-in for boost::dynamic_bitset of
make_golden_consensus.py.  The vectors are therefore "probe with substitutes".  Only inputs (the two mates, the settings)
and results (merged or not, the offset, the merged strings) are stored; no reference source is.

min_score (0.99) and min_overlap (15) are constants of the reference's function (:873-874); every case has them.

    python tests/golden/make_golden_self_overlap.py          writes the file
    python tests/golden/make_golden_self_overlap.py --time   times the probe on 2,000 pairs of 2 x 150 that do not overlap
                                                             (tools/self_overlap_bench.py's first workload), one thread
"""
import ctypes as C
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

SHELL_HEAD = r"""
#include <assert.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <iostream>
#include <list>
#include <string>
#include <unordered_map>
#include <vector>
#include "Read.h"
#include "Types.h"
namespace boost {
template <typename T = unsigned long>
class dynamic_bitset {
    std::vector<unsigned char> v;
public:
    explicit dynamic_bitset(size_t n) : v(n, 0) {}
    unsigned char& operator[](size_t i) { return v[i]; }
    size_t count() const { size_t c = 0; for (unsigned char b : v) c += b != 0; return c; }
};
}
class EdgeCalculator {
public:
    ProgramSettings program_settings;
    double score(char nt1, char nt2, double p1, double p2, int & mismatch_count);
    double phred_to_prob(const int phred);
    double overlap_score(std::string seq1, std::string seq2, std::string score1, std::string score2, const unsigned int pos, double & mismatch_rate);
};
class SRBuilder {
public:
    double minQual;
    ProgramSettings program_settings;
    double phred_to_prob(const int phred);
    bool consensus_pos(std::string nucleotides, std::string qualities, std::string &cons_seq, std::string& cons_qual);
    int consensus(int total_len, std::list<int> &pos_list, std::list<std::string> &seq_list, std::list<std::string> &qual_list,
                  std::string &cons_seq, std::string &cons_qual, bool subreads_needed, bool error_correction);
    Read merge_self_overlap(Read superread, EdgeCalculator & edge_calculator);
};
"""

SHELL_TAIL = r"""
extern "C" int probe_merge(const char* s1, const char* q1, const char* s2, const char* q2, double mismatch, unsigned int min_read_len,
                           double min_qual, char* out_seq, char* out_qual, int* out_len) {
    SRBuilder b;
    b.minQual = min_qual;
    b.program_settings.min_clique_size = 2;
    EdgeCalculator ec;
    ec.program_settings.mismatch = mismatch;
    ec.program_settings.min_read_len = min_read_len;
    Read r(true, true, 7, s1, s2, q1, q2);
    Read m = b.merge_self_overlap(r, ec);
    if (m.is_paired()) return 0;
    std::string cs = m.get_seq(0), cq = m.get_phred(0);
    if (cs.size() != cq.size()) return -1000;
    memcpy(out_seq, cs.data(), cs.size());
    memcpy(out_qual, cq.data(), cq.size());
    *out_len = (int)cs.size();
    return 1;
}
"""


def build_probe(tmp):
    src = os.path.join(tmp, "probe.cpp")
    sr = open(os.path.join(REF, "SRBuilder.cpp")).read().split("\n")
    ec = open(os.path.join(REF, "EdgeCalculator.cpp")).read().split("\n")
    with open(src, "w") as f:
        f.write(SHELL_HEAD)
        f.write("\n".join(ec[25:139]) + "\n")
        f.write("\n".join(sr[288:535]) + "\n")
        f.write("\n".join(sr[871:955]) + "\n")
        f.write(SHELL_TAIL)
    so = os.path.join(tmp, "probe.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-I", REF, "-o", so, src], check=True)
    dll = C.CDLL(so)
    dll.probe_merge.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_double, C.c_uint, C.c_double, C.c_char_p, C.c_char_p,
                                C.POINTER(C.c_int)]
    return dll


def run(dll, c):
    cap = len(c["seq1"]) + len(c["seq2"]) + 8
    o1, o2, ol = C.create_string_buffer(cap), C.create_string_buffer(cap), C.c_int(0)
    r = dll.probe_merge(c["seq1"].encode(), c["qual1"].encode(), c["seq2"].encode(), c["qual2"].encode(), c["mismatch"], c["min_read_len"],
                        c["min_qual"], o1, o2, C.byref(ol))
    assert r in (0, 1)
    return r, o1.raw[:ol.value].decode(), o2.raw[:ol.value].decode()


class quiet:  # the reference prints (pos beyond the sequence, p_incorrect NaN)
    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        dn = os.open(os.devnull, os.O_WRONLY)
        os.dup2(dn, 1)
        os.close(dn)

    def __exit__(self, *a):
        os.dup2(self.saved, 1)
        os.close(self.saved)


def no_overlap_pairs(n, length, seed):
    """pairs whose mates come from unrelated places of a random genome: the whole scan, nothing merges"""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(20000))
    qs = [chr(33 + q) for q in (2, 14, 22, 27, 33, 37, 40)]
    out = []
    for _ in range(n):
        a, b = rng.randrange(0, 9000), rng.randrange(10000, 19000)
        out.append((genome[a:a + length], "".join(rng.choice(qs) for _ in range(length)), genome[b:b + length],
                    "".join(rng.choice(qs) for _ in range(length))))
    return out


def main():
    rng = random.Random(20240917)
    genome = "".join(rng.choice("ACGT") for _ in range(6000))
    qchars = "".join(chr(33 + q) for q in (2, 11, 15, 20, 25, 30, 33, 37, 38, 39, 40, 41))
    cases = []

    def qual(n, lo=3):
        return "".join(rng.choice(qchars[lo:]) for _ in range(n))

    def noisy(s, rate):
        return "".join(rng.choice("ACGT") if rng.random() < rate else c for c in s)

    def case(name, s1, q1, s2, q2, mismatch=(0.0,), min_read_len=(0,), min_qual=(0.99,)):
        assert len(s1) == len(q1) and len(s2) == len(q2) and s1 and s2
        for mm in mismatch:
            for mrl in min_read_len:
                for mq in min_qual:
                    cases.append(dict(name=f"{name}/mm{mm}/mrl{mrl}/mq{mq}", seq1=s1, qual1=q1, seq2=s2, qual2=q2, mismatch=mm, min_read_len=mrl,
                                      min_qual=mq))

    def overlapping(name, a, l1, p, l2, rate=0.0, **kw):
        """mate 1 = genome[a : a + l1], mate 2 starts p bases into it"""
        case(name, noisy(genome[a:a + l1], rate), qual(l1), noisy(genome[a + p:a + p + l2], rate), qual(l2), **kw)

    # L1 around min_overlap: 14 and 15 have no offset at all, 16 has p = 1, 17 has p = 2, 1
    for l1 in (14, 15, 16, 17):
        overlapping(f"l1_{l1}_hit_p1", 100, l1, 1, 20)
        overlapping(f"l1_{l1}_identical", 100, l1, 0, l1)
        case(f"l1_{l1}_unrelated", genome[200:200 + l1], qual(l1), genome[900:930], qual(30))
    # L1 - 15 offsets at the chunk boundaries of the device's scan: no hit (the whole scan), a hit at p = 1, at p = L1 - 15, in between
    for k in (63, 64, 65, 128, 129, 256, 257):
        l1 = k + 15
        case(f"offsets_{k}_none", genome[300:300 + l1], qual(l1), genome[2000:2000 + 90], qual(90))
        overlapping(f"offsets_{k}_p1", 300, l1, 1, 60)
        overlapping(f"offsets_{k}_pmax", 300, l1, k, 40)
        overlapping(f"offsets_{k}_mid", 300, l1, k // 2 + 1, 200, rate=0.002)
    # L2 = 1: a one-base mate 2 matches wherever mate 1 has its base
    case("l2_1", genome[500:560], qual(60), genome[520], "I")
    case("l2_1_n", genome[500:560], qual(60), "N", "I")
    case("l2_2", genome[500:560], qual(60), genome[530:532], "II")
    # mate 2 contained in mate 1: total_len = L2 + p < L1, the output stops there
    overlapping("contained", 600, 120, 30, 40)
    overlapping("contained_p1", 600, 120, 1, 20)
    overlapping("contained_to_end", 600, 120, 100, 20)
    # two qualifying offsets: a repeat of period 20 — the larger offset wins
    unit = genome[700:720]
    case("two_offsets", genome[650:700] + unit * 3, qual(110), unit * 2 + genome[3000:3030], qual(70))
    case("homopolymer", "A" * 80, qual(80), "A" * 50, qual(50))
    # runs of N: overlaps without a counted position score 0
    s1 = genome[800:860] + "N" * 40
    case("n_run_tail", s1, qual(100), genome[2100:2130], qual(30))
    case("n_run_both", "N" * 60, qual(60), "N" * 40, qual(40))
    case("n_run_then_hit", genome[800:860] + "N" * 25, qual(85), "N" * 10 + genome[855:900], qual(55))
    # N inside a hit (in either mate, in both at one column)
    a, b = list(genome[1000:1100]), list(genome[1060:1160])
    for i in (62, 70, 95):
        a[i] = "N"
    for i in (3, 10, 35):
        b[i] = "N"
    case("n_inside_hit", "".join(a), qual(100), "".join(b), qual(100), min_qual=(0.9, 0.99))
    # --mismatch: a low-quality mismatch whose probability lies below 0.01 kills the offset that would otherwise pass
    m1, m2 = genome[1200:1300], list(genome[1250:1350])
    m2[20] = "A" if m2[20] != "A" else "C"
    q1, q2 = "I" * 100, "I" * 100
    case("mismatch_setting_hiq", m1, q1, "".join(m2), q2, mismatch=(0.0, 0.01))
    # (one mismatch of two Q2 bases, p = 0.24: 400 matching positions around it keep the mean above log 0.99; --mismatch 0.3 rejects the offset)
    w1, w2 = genome[1200:1650], list(genome[1250:1700])
    w2[20] = "A" if w2[20] != "A" else "C"
    case("mismatch_setting_loq", w1, "I" * 70 + "#" + "I" * 379, "".join(w2), "I" * 20 + "#" + "I" * 429, mismatch=(0.0, 0.01, 0.3))
    overlapping("mismatch_setting_noisy", 1200, 150, 60, 150, rate=0.01, mismatch=(0.0, 0.01))
    # --min_read_len above one mate's length: every offset scores 0
    overlapping("min_read_len", 1400, 100, 40, 80, min_read_len=(0, 80, 81, 100, 101))
    # min_qual 0.9 / 0.99 on an overlap with disagreeing low-quality bases
    lo = "".join(rng.choice("+5?I") for _ in range(120))
    case("min_qual", noisy(genome[1500:1620], 0.004), lo, noisy(genome[1560:1680], 0.004), lo[::-1], min_qual=(0.9, 0.99))
    # every quality byte 33 .. 126 in one pair
    allq = "".join(chr(b) for b in range(33, 127))
    case("all_phred", genome[1700:1794], allq, genome[1750:1844], allq[::-1], min_qual=(0.9, 0.99))
    case("all_phred_shift", genome[1700:1794] * 2, allq + allq[47:] + allq[:47], genome[1780:1794] + genome[1700:1780], allq[31:] + allq[:31])
    hiq = "".join(chr(rng.randrange(93, 127)) for _ in range(94))
    case("all_phred_high", genome[1700:1794], hiq, genome[1730:1824], hiq[::-1])
    # excerpts of the committed SAVAGE mates, cut so that some truly overlap: mate 1 = the read's first bases, mate 2 = a later window of
    # the SAME read with the other file's qualities (a true overlap), or the other mate as it is (none)
    p1 = gzip.open(os.path.join(ROOT, "tests", "golden", "savage_paired1.fastq.gz"), "rt").read().split("\n")
    p2 = gzip.open(os.path.join(ROOT, "tests", "golden", "savage_paired2.fastq.gz"), "rt").read().split("\n")
    for i in range(8):
        s, q, t, u = p1[4 * i + 1], p1[4 * i + 3], p2[4 * i + 1], p2[4 * i + 3]
        n = min(len(s), len(u))
        case(f"savage_{i}_true", s[:120], q[:120], s[70:n], u[70:n], min_qual=(0.9, 0.99))
        case(f"savage_{i}_mates", s[:120], q[:120], t[:110], u[:110])
    # random pairs: lengths 16 .. 300, 1 % substitutions, about half overlapping
    for i in range(40):
        l1, l2 = rng.randrange(16, 301), rng.randrange(16, 301)
        a = rng.randrange(0, 2000)
        if i % 2:
            p = rng.randrange(1, l1)
            s2 = genome[a + p:a + p + l2]
        else:
            s2 = genome[3000 + a:3000 + a + l2]
        nrate = 0.02 if i % 5 == 0 else 0.0
        s1 = "".join("N" if rng.random() < nrate else c for c in noisy(genome[a:a + l1], 0.01))
        case(f"random_{i}", s1, qual(l1, lo=0), noisy(s2, 0.01), qual(l2, lo=0), mismatch=(0.0, 0.01))

    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        if "--time" in sys.argv:
            pairs = no_overlap_pairs(2000, 150, 7)
            with quiet():
                t0 = time.perf_counter()
                n_merged = 0
                for s1, q1, s2, q2 in pairs:
                    n_merged += run(dll, dict(seq1=s1, qual1=q1, seq2=s2, qual2=q2, mismatch=0.0, min_read_len=0, min_qual=0.99))[0]
                dt = time.perf_counter() - t0
            print(json.dumps(dict(workload="2000 pairs of 2 x 150, none overlapping", threads=1, seconds=dt, pairs_per_s=2000 / dt, merged=n_merged)))
            return
        with quiet():
            for c in cases:
                r, cs, cq = run(dll, c)
                c.update(merged=r, overlap_pos=(len(cs) - len(c["seq2"])) if r else -1, merged_seq=cs, merged_qual=cq)
    n_merged = sum(c["merged"] for c in cases)
    assert 0.25 * len(cases) < n_merged < 0.75 * len(cases), (n_merged, len(cases))
    by = {c["name"].split("/")[0]: c for c in cases}
    assert by["contained"]["merged"] and len(by["contained"]["merged_seq"]) < 120
    assert by["two_offsets"]["overlap_pos"] == 90, by["two_offsets"]["overlap_pos"]
    assert not by["l1_15_hit_p1"]["merged"] and by["l1_16_hit_p1"]["overlap_pos"] == 1
    out = dict(provenance="probe with substitutes: src/SRBuilder.cpp:872-955 and :289-535, src/EdgeCalculator.cpp:26-139 with the genuine Read.h / "
                          "Types.h in declaration shells for SRBuilder and EdgeCalculator, boost::dynamic_bitset replaced by a stand-in",
               min_score=0.99, min_overlap=15, cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "self_overlap.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(f"{len(cases)} cases, {n_merged} merged, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
