#!/usr/bin/env python3
"""Generates tests/golden/consensus.json with the reference's own SRBuilder::consensus / consensus_pos.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory:
src/SRBuilder.cpp:289-535 (phred_to_prob, consensus_pos, consensus) streamed from the reference by line range into a
build-owned declaration shell (below): a class with the members the text uses (minQual,
program_settings.min_clique_size) and a few-line stand-in for boost::dynamic_bitset with operator[] and count() —
Boost is not available to the probe.  The vectors are therefore "probe with substitutes".  Only inputs (reads, layouts,
settings) and results (return value, cons_seq, cons_qual) are stored; no reference source is.

The status of a case is not something the reference returns: the four empty results share return values.  Each case
states the exit it was built to take; the generator checks that against what the probe can tell (return value, empty
or not, the "NaN" / "Not enough support" lines).
"""
import ctypes as C
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"
OK, NO_SUPPORT, MEMBER_SHORT, UNCOVERED, NAN = 0, 1, 2, 3, 4

SHELL_HEAD = r"""
#include <assert.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <iostream>
#include <list>
#include <string>
#include <vector>
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
struct ProbeSettings { unsigned int min_clique_size; };
class SRBuilder {
public:
    double minQual;
    ProbeSettings program_settings;
    double phred_to_prob(const int phred);
    bool consensus_pos(std::string nucleotides, std::string qualities, std::string &cons_seq, std::string& cons_qual);
    int consensus(int total_len, std::list<int> &pos_list, std::list<std::string> &seq_list, std::list<std::string> &qual_list,
                  std::string &cons_seq, std::string &cons_qual, bool subreads_needed, bool error_correction);
};
"""

SHELL_TAIL = r"""
extern "C" int probe_consensus(int total_len, int n, const int* pos, const char** seqs, const char** quals, int subreads_needed,
                               int error_correction, double min_qual, unsigned int min_clique_size, char* out_seq, char* out_qual, int* out_len) {
    SRBuilder b;
    b.minQual = min_qual;
    b.program_settings.min_clique_size = min_clique_size;
    std::list<int> pos_list(pos, pos + n);
    std::list<std::string> seq_list, qual_list;
    for (int i = 0; i < n; i++) { seq_list.push_back(seqs[i]); qual_list.push_back(quals[i]); }
    std::string cs, cq;
    int r = b.consensus(total_len, pos_list, seq_list, qual_list, cs, cq, subreads_needed != 0, error_correction != 0);
    if (cs.size() != cq.size()) return -1000;
    memcpy(out_seq, cs.data(), cs.size());
    memcpy(out_qual, cq.data(), cq.size());
    *out_len = (int)cs.size();
    return r;
}
"""


def build_probe(tmp):
    src = os.path.join(tmp, "probe.cpp")
    lines = open(os.path.join(REF, "SRBuilder.cpp")).read().split("\n")
    with open(src, "w") as f:
        f.write(SHELL_HEAD)
        f.write("\n".join(lines[288:535]) + "\n")
        f.write(SHELL_TAIL)
    so = os.path.join(tmp, "probe.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def oriented(read, seq, rev):
    s, q = read[0 if seq in (0, 1) else 1]
    return ("".join(COMP[c] for c in reversed(s)), q[::-1]) if rev else (s, q)


def run(dll, reads, case):
    ms = case["members"]
    n = len(ms)
    strs = [oriented(reads[m["read"]], m["seq"], m["rev"]) for m in ms]
    pos = (C.c_int * n)(*[m["pos"] for m in ms])
    seqs = (C.c_char_p * n)(*[s.encode() for s, _ in strs])
    quals = (C.c_char_p * n)(*[q.encode() for _, q in strs])
    cap = max(case["total_len"], 1) + 8
    o1, o2, ol = C.create_string_buffer(cap), C.create_string_buffer(cap), C.c_int(0)
    st = case["settings"]
    dll.probe_consensus.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_uint, C.c_char_p,
                                    C.c_char_p, C.POINTER(C.c_int)]
    r = dll.probe_consensus(case["total_len"], n, pos, seqs, quals, st["subreads_needed"], st["error_correction"], st["min_qual"],
                            st["min_clique_size"], o1, o2, C.byref(ol))
    assert r != -1000
    return r, o1.raw[:ol.value].decode(), o2.raw[:ol.value].decode()


class Builder:
    def __init__(self):
        self.reads = []  # each: [[seq, qual]] or [[seq1, qual1], [seq2, qual2]]
        self.cases = []

    def read(self, seq, qual):
        assert len(seq) == len(qual) and len(seq) > 0
        self.reads.append([[seq, qual]])
        return len(self.reads) - 1

    def pair(self, s1, q1, s2, q2):
        self.reads.append([[s1, q1], [s2, q2]])
        return len(self.reads) - 1

    def case(self, name, members, total_len=None, expect=OK, ec=(0, 1), min_qual=(0.99,), mcs=(2,), subreads=(0,)):
        """members: (read, seq, rev, pos); total_len defaults to the furthest end"""
        ms = [dict(read=r, seq=s, rev=v, pos=p) for r, s, v, p in members]
        if total_len is None:
            total_len = max(m["pos"] + len(self.reads[m["read"]][0 if m["seq"] in (0, 1) else 1][0]) for m in ms)
        exp = expect if isinstance(expect, dict) else None
        for e in ec:
            for mq in min_qual:
                for k in mcs:
                    for sn in subreads:
                        key = (e, k, sn)
                        status = exp.get(key, exp.get(e, OK)) if exp else expect
                        if e and len(ms) < (2 if sn else k):  # :430-446
                            status = NO_SUPPORT
                        self.cases.append(dict(name=f"{name}/ec{e}/mq{mq}/mcs{k}/sub{sn}", total_len=total_len, members=ms,
                                               settings=dict(min_qual=mq, min_clique_size=k, error_correction=e, subreads_needed=sn),
                                               status=status))


def noisy(rng, s, rate):
    return "".join(rng.choice("ACGT") if rng.random() < rate else c for c in s)


def main():
    rng = random.Random(20240611)
    B = Builder()
    genome = "".join(rng.choice("ACGT") for _ in range(2000))
    qchars = "".join(chr(33 + q) for q in (2, 11, 15, 20, 25, 30, 33, 37, 38, 39, 40, 41))

    def qual(n, lo=0):
        return "".join(rng.choice(qchars[lo:]) for _ in range(n))

    def window(a, n, rate=0.01, nrate=0.0, lo=0):
        s = noisy(rng, genome[a:a + n], rate)
        s = "".join("N" if rng.random() < nrate else c for c in s)
        return B.read(s, qual(n, lo))

    # depth 1, 2, 3, 8, 40: synthetic tilings (step positions, both orientations)
    for depth, step, n in ((1, 0, 60), (2, 25, 60), (3, 17, 60), (8, 9, 70), (40, 3, 80)):
        ms = []
        for i in range(depth):
            rev = i % 3 == 1
            a = 100 + i * step
            r = window(a, n)
            if rev:  # store the reverse complement so that the oriented member reads the genome
                s, q = B.reads[r][0]
                B.reads[r][0] = ["".join(COMP[c] for c in reversed(s)), q[::-1]]
            ms.append((r, 0, int(rev), i * step))
        # (fewer members than min_clique_size under error correction: "Not enough support")
        B.case(f"tiling_d{depth}", ms, mcs=(2, 4), min_qual=(0.9, 0.99))
        if depth == 3:
            B.case("tiling_d3_subreads", ms, mcs=(4,), subreads=(1,))  # subreads_needed: minimumSupport = 2
    # members from the committed FASTQ excerpts (truncated to 90 bases; they do not agree: plenty of close calls)
    fq = gzip.open(os.path.join(ROOT, "tests", "golden", "savage_singles.fastq.gz"), "rt").read().split("\n")
    ex = [B.read(fq[4 * i + 1][:90], fq[4 * i + 3][:90]) for i in range(12)]
    B.case("excerpt_d2", [(ex[0], 0, 0, 0), (ex[1], 0, 1, 30)])
    B.case("excerpt_same_d3", [(ex[2], 0, 0, 0), (ex[2], 0, 0, 0), (ex[2], 0, 0, 5)], total_len=95)
    B.case("excerpt_d8", [(ex[i], 0, i & 1, 7 * i) for i in range(8)], mcs=(2, 4))
    pq = gzip.open(os.path.join(ROOT, "tests", "golden", "savage_paired1.fastq.gz"), "rt").read().split("\n")
    pr = gzip.open(os.path.join(ROOT, "tests", "golden", "savage_paired2.fastq.gz"), "rt").read().split("\n")
    pp = [B.pair(pq[4 * i + 1][:80], pq[4 * i + 3][:80], pr[4 * i + 1][:70], pr[4 * i + 3][:70]) for i in range(3)]
    B.case("excerpt_pairs", [(pp[0], 1, 0, 0), (pp[1], 2, 1, 10), (pp[2], 1, 1, 20), (pp[0], 2, 0, 40)], mcs=(2, 4))
    # N in one member, in all members
    a = B.read("ACGTNACGTNACGTACGTAC", "IIII!IIIIIIIIIIIIIII")
    b = B.read("ACGTAACGTNACGTACGTAC", "IIIIIIIII5IIIIIIIIII")
    c = B.read("NNNNNNNNNN", "IIIII!!!!!")
    B.case("n_one_member", [(a, 0, 0, 0), (b, 0, 0, 0)])
    B.case("n_three", [(a, 0, 0, 0), (b, 0, 0, 0), (a, 0, 0, 0)])
    B.case("n_all_members", [(c, 0, 0, 0), (c, 0, 1, 0), (c, 0, 0, 0)])
    B.case("n_alone", [(c, 0, 0, 0)], ec=(0,))
    B.case("n_first_then_base", [(c, 0, 0, 0), (a, 0, 0, 0)], total_len=20)
    # equal scores for two bases: same quality, different base (tie order A, T, C, G)
    for x, y in ("AT", "TA", "AC", "CA", "AG", "TC", "CT", "TG", "GT", "CG", "GC"):
        r1, r2 = B.read(x * 6, "5I+!~#"), B.read(y * 6, "5I+!~#")
        B.case(f"tie_{x}{y}", [(r1, 0, 0, 0), (r2, 0, 0, 0)], ec=(0,), min_qual=(0.99, 0.3))
    t4 = [B.read(x * 4, "5555") for x in "GCTA"]
    B.case("tie_four", [(r, 0, 0, 0) for r in t4], ec=(0,), min_qual=(0.99, 0.2))
    # qualities that reach the 93 clamp, and low ones that the minQual rule rejects
    hi = [B.read(genome[300:340], "~" * 40), B.read(genome[300:340], "I" * 40), B.read(genome[300:340], "I" * 40)]
    B.case("clamp93_d1", [(hi[0], 0, 0, 0)], ec=(0,))
    B.case("clamp93_d2", [(hi[1], 0, 0, 0), (hi[2], 0, 0, 0)])
    B.case("clamp93_d3", [(hi[0], 0, 0, 0), (hi[1], 0, 0, 0), (hi[2], 0, 0, 0)])
    lo = [B.read(noisy(rng, genome[300:340], 0.3), "".join(rng.choice("\"#$%&'(") for _ in range(40))) for _ in range(4)]
    B.case("lowqual_reject", [(r, 0, 0, 0) for r in lo], min_qual=(0.9, 0.99))
    B.case("lowqual_d2", [(lo[0], 0, 0, 0), (lo[1], 0, 0, 3)], min_qual=(0.9, 0.99))
    # a member shorter than its trimmed start (error correction: trim_pos = the second position)
    s1, s2, s3 = B.read(genome[400:405], "IIIII"), window(400, 60), window(420, 60)
    B.case("member_short", [(s1, 0, 0, 0), (s2, 0, 0, 0), (s3, 0, 0, 20)], expect={1: MEMBER_SHORT}, mcs=(3,))
    # a gap nobody covers
    g1, g2, g3 = window(500, 30), window(540, 30), window(545, 30)
    B.case("gap", [(g1, 0, 0, 0), (g2, 0, 0, 40), (g3, 0, 0, 45)], expect={0: UNCOVERED, 1: MEMBER_SHORT})
    B.case("gap_after_trim", [(g1, 0, 0, 0), (g1, 0, 0, 0), (g2, 0, 0, 40), (g3, 0, 0, 45)], expect={0: UNCOVERED, 1: UNCOVERED})
    B.case("gap_at_end", [(g1, 0, 0, 0), (g2, 0, 0, 10)], total_len=50, expect={0: UNCOVERED, 1: OK})
    # suffix cut; a low-support column in the middle (kept, not cut)
    m1, m2, m3, m4 = window(600, 40), window(610, 20), window(635, 40), window(640, 50)
    B.case("suffix_cut", [(m1, 0, 0, 0), (m2, 0, 0, 10), (m4, 0, 0, 12)], mcs=(2, 3))
    B.case("low_support_middle", [(m1, 0, 0, 0), (m2, 0, 0, 10), (m3, 0, 0, 35), (m4, 0, 0, 40)], mcs=(2,))
    B.case("equal_positions", [(m1, 0, 0, 0), (m3, 0, 0, 0), (m2, 0, 0, 0), (m4, 0, 0, 7)], mcs=(2, 4))
    # every Phred byte from '!' to '~' at depth 1 and in pairs
    allq = "".join(chr(b) for b in range(33, 127))
    qa = B.read((genome[700:794]), allq)
    B.case("all_phred_d1", [(qa, 0, 0, 0)], ec=(0,))
    for k, shift in enumerate((0, 1, 7, 31, 47, 60, 93)):
        qb = B.read(genome[700:794] if k % 2 == 0 else noisy(rng, genome[700:794], 0.5), allq[shift:] + allq[:shift])
        B.case(f"all_phred_pairs_{shift}", [(qa, 0, 0, 0), (qb, 0, 0, 0)], ec=(0,), min_qual=(0.9, 0.99))
        B.case(f"all_phred_pairs_rev_{shift}", [(qb, 0, 0, 0), (qa, 0, 0, 0)], ec=(0,))
    # random cliques: mixed lengths, random qualities over the whole range, Ns
    for i in range(12):
        depth = rng.choice((3, 4, 5, 8, 13))
        pos, ms = 0, []
        for j in range(depth):
            n = rng.randrange(20, 70)
            r = window(800 + pos, n, rate=0.05, nrate=0.03)
            if i % 3 == 0:
                B.reads[r][0][1] = "".join(chr(rng.randrange(33, 127)) for _ in range(n))
            ms.append((r, 0, 0, pos))
            pos += rng.randrange(0, 12)
        B.case(f"random_{i}", ms, expect=None, mcs=(2, 4))

    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        sys.stdout.flush()
        devnull = os.open(os.devnull, os.O_WRONLY)
        saved = os.dup(1)
        os.dup2(devnull, 1)  # the reference prints per exit
        try:
            for case in B.cases:
                r, cs, cq = run(dll, B.reads, case)
                case.update(ret=r, cons_seq=cs, cons_qual=cq)
        finally:
            os.dup2(saved, 1)
    for case in B.cases:
        r, cs = case["ret"], case["cons_seq"]
        if case["status"] is None:  # random layouts: the status as far as the probe tells it apart
            case["status"] = NO_SUPPORT if r == -1 else (OK if (cs or r != 0) else None)
            if case["status"] is None:
                case["status"] = -1  # empty with return value 0: the test accepts any of the statuses that return 0
            continue
        s = case["status"]
        if s == NO_SUPPORT:
            assert r == -1 and cs == "", case["name"]
        elif s in (MEMBER_SHORT, UNCOVERED):
            assert r == 0 and cs == "", (case["name"], r, cs)
        else:
            assert r >= 0 and cs != "", (case["name"], r)
    out = dict(provenance="probe with substitutes: src/SRBuilder.cpp:289-535 in a declaration shell, boost::dynamic_bitset replaced by a stand-in",
               reads=B.reads, cases=B.cases)
    path = os.path.join(ROOT, "tests", "golden", "consensus.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(f"{len(B.cases)} cases, {len(B.reads)} reads, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
