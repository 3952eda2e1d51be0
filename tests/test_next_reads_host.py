"""hc_host_sr_next_reads (include/hcsr.h) against a Python restatement of the reference lines it cites, written here: which super-reads
survive process_cliques (src/SRBuilder.cpp:983,986-996,999-1001), Read::get_len / test_N_rate (src/Read.h:203-234), the trivial
super-reads with their reversal (src/SRBuilder.cpp:1282-1372) and the numbering across the groups.  No reference code runs: the names say
"restatement".  build_rev_comp's mapping is the one tests/golden/ref_headers.json pins."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import next_reads as NR
from haploconduct_amd.readstore import ReadSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REV_COMP = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_headers.json")))["rev_comp"]
COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N"}


def _test_n_rate(seq):  # src/Read.h:214-234 on the concatenation
    return float(seq.count(b"N")) < 0.05 * float(len(seq))


def restatement(reads, cons_seq, cons_qual, entries, extra_seq=b"", extra_qual=b"", keep_singletons=0):
    """-> (new_id, status, [read]) with read = [(seq, qual)] of one or two mates."""
    src = {NR.SRC_CONSENSUS: (bytes(cons_seq), bytes(cons_qual)), NR.SRC_BYTES: (bytes(extra_seq), bytes(extra_qual))}
    new_id, status, out = [], [], []
    for e in entries:
        kind, rev = int(e["kind"]), int(e["rev"])
        st, mates = NR.NEXT_KEPT, []
        if kind > NR.NEXT_TRIVIAL_PAIRED or rev > 1:
            st = NR.NEXT_BAD_ENTRY
        elif kind in (NR.NEXT_SINGLE, NR.NEXT_PAIRED):
            for k in range(1 + (kind == NR.NEXT_PAIRED)):
                s, off, ln = int(e["src%d" % (k + 1)]), int(e["off%d" % (k + 1)]), int(e["len%d" % (k + 1)])
                if s not in src or ln >= 1 << 28 or off + ln > len(src[s][0]):
                    st = NR.NEXT_BAD_ENTRY
                    break
                mates.append((src[s][0][off:off + ln], src[s][1][off:off + ln]))
            if st == NR.NEXT_KEPT and any(len(m[0]) == 0 for m in mates):  # :983, :999
                st = NR.NEXT_DROPPED_EMPTY
        else:
            r = int(e["read"])
            if reads is None or r >= reads.n_reads or reads.is_paired(r) != (kind == NR.NEXT_TRIVIAL_PAIRED):
                st = NR.NEXT_BAD_ENTRY
            else:
                q0 = int(reads.read_first_seq[r])
                mates = [reads.seq(q0 + k) for k in range(1 + reads.is_paired(r))]
                if sum(len(m[0]) for m in mates) < keep_singletons:  # :1286, before the N rate (:1292; the count is the same reversed)
                    st = NR.NEXT_DROPPED_SHORT
                elif rev:  # :1342, :1355
                    mates = [(bytes(COMP.get(chr(b), chr(b)).encode()[0] for b in s[::-1]), q[::-1]) for s, q in mates[::-1]]
        if st == NR.NEXT_KEPT and not _test_n_rate(b"".join(m[0] for m in mates)):
            st = NR.NEXT_DROPPED_N_RATE
        status.append(st)
        new_id.append(len(out) if st == NR.NEXT_KEPT else -1)
        if st == NR.NEXT_KEPT:
            out.append(mates)
    return new_id, status, out


def _as_lists(rs):
    return [[rs.seq(q) for q in range(int(rs.read_first_seq[r]), int(rs.read_first_seq[r + 1]))] for r in range(rs.n_reads)]


def _check(reads, cons, entries, extra=(b"", b""), keep_singletons=0):
    entries = np.array(entries, NR.NEXT_ENTRY_DTYPE)
    cs, cq = cons
    got = NR.host_next_reads(reads, np.frombuffer(cs, np.uint8), np.frombuffer(cq, np.uint8), entries, np.frombuffer(extra[0], np.uint8),
                             np.frombuffer(extra[1], np.uint8), keep_singletons)
    new_id, status, out = restatement(reads, cs, cq, entries, extra[0], extra[1], keep_singletons)
    assert got.status.tolist() == status and got.new_id.tolist() == new_id
    assert got.empty == (len(out) == 0)
    if out:
        assert _as_lists(got.reads) == out
        assert got.counts["n_kept"] == len(out) and got.counts["n_seq"] == sum(len(m) for m in out)
    return got


def _q(n, c=b"I"):
    return c * n


def test_restatement_n_rate_boundary():
    # 20 bases with one N: 1 < 0.05 * 20 = 1.0 is false; 21 with one N: kept; a single base; an N alone
    cs = b"N" + b"A" * 19 + b"N" + b"C" * 20 + b"G" + b"N"
    cq = _q(len(cs))
    got = _check(None, (cs, cq), [NR.single(0, 20), NR.single(20, 21), NR.single(41, 1), NR.single(42, 1),
                                  # pairs: counts and lengths of the concatenation — 10 + 10 with one N is dropped, 10 + 11 is kept
                                  NR.paired(0, 10, 21, 10), NR.paired(0, 10, 21, 11),
                                  # a mate that alone would fail (N + 9 bases) passes with a long enough partner
                                  NR.paired(0, 10, 21, 20)])
    assert got.status.tolist() == [2, 0, 0, 2, 2, 0, 0]


def test_restatement_pair_with_an_empty_mate_is_dropped_whole():
    cs = b"ACGTACGTAC"
    got = _check(None, (cs, _q(10)), [NR.paired(0, 5, 5, 0), NR.paired(0, 0, 5, 5), NR.single(3, 0), NR.paired(0, 5, 5, 5)])
    assert got.status.tolist() == [1, 1, 1, 0] and got.new_id.tolist() == [-1, -1, -1, 0]
    assert got.reads.n_reads == 1 and got.reads.n_seq == 2


def _store():
    singles = [(v["seq"], "".join(chr(40 + (i * 7 + k) % 50) for k in range(len(v["seq"])))) for i, v in enumerate(REV_COMP)]
    pairs = [((REV_COMP[i]["seq"], "5" * len(REV_COMP[i]["seq"])), (REV_COMP[i + 1]["seq"], "".join(chr(60 + k % 30) for k in range(len(REV_COMP[i + 1]["seq"])))))
             for i in range(0, len(REV_COMP) - 1, 2)]
    return ReadSet.from_lists(singles, pairs), len(singles), len(pairs)


def test_restatement_keep_singletons_is_tested_against_len1_plus_len2():
    reads = ReadSet.from_lists([("ACGTA", "IIIII"), ("ACGTAC", "IIIIII")], [(("ACG", "III"), ("TTTT", "IIII")), (("ACG", "III"), ("TT", "II"))])
    got = _check(reads, (b"", b""), [NR.trivial(0), NR.trivial(1), NR.trivial(2, is_paired=True), NR.trivial(3, is_paired=True)], keep_singletons=6)
    assert got.status.tolist() == [3, 0, 0, 3]
    # a short read that also fails the N rate is "short": the length is tested first (:1286, :1292)
    reads = ReadSet.from_lists([("NN", "II")])
    assert _check(reads, (b"", b""), [NR.trivial(0)], keep_singletons=3).status.tolist() == [3]
    assert _check(reads, (b"", b""), [NR.trivial(0)], keep_singletons=2).status.tolist() == [2]


def test_restatement_reverse_trivials_against_the_golden_rev_comp_vectors():
    reads, n_s, n_p = _store()
    assert n_s >= 5 and n_p >= 2
    entries = [NR.trivial(r, rev=True) for r in range(n_s)] + [NR.trivial(n_s + p, rev=True, is_paired=True) for p in range(n_p)] + \
              [NR.trivial(r) for r in range(n_s)] + [NR.trivial(n_s + p, is_paired=True) for p in range(n_p)]
    got = NR.host_next_reads(reads, None, None, np.array(entries, NR.NEXT_ENTRY_DTYPE))
    kept = _as_lists(got.reads)
    for r, v in enumerate(REV_COMP):
        if got.status[r] != NR.NEXT_KEPT:
            assert not _test_n_rate(v["seq"].encode())
            continue
        (s, q), = kept[got.new_id[r]]
        assert s.decode() == v["rev_comp"] and q == reads.seq(r)[1][::-1]
    n_checked = 0
    for p in range(n_p):
        i = n_s + p
        if got.status[i] != NR.NEXT_KEPT:
            continue
        (s1, q1), (s2, q2) = kept[got.new_id[i]]  # (rev_comp(2), rev_comp(1)) with the reversed Phred strings
        assert s1.decode() == REV_COMP[2 * p + 1]["rev_comp"] and s2.decode() == REV_COMP[2 * p]["rev_comp"]
        assert q1 == reads.seq(n_s + 2 * p + 1)[1][::-1] and q2 == reads.seq(n_s + 2 * p)[1][::-1]
        n_checked += 1
    assert n_checked >= 1
    _check(reads, (b"", b""), entries)  # and the forward ones, with the numbering, against the restatement


def test_restatement_numbering_runs_across_the_three_groups_with_drops_in_each():
    reads = ReadSet.from_lists([("ACGTACGTACGTACGTACGTACG", _q(23).decode()), ("NNNNACGT", "IIIIIIII"), ("ACGTTGCAACGTTGCAACGTTGCA", _q(24, b"5").decode())],
                               [(("ACGTACGTACGTACGTACGTA", _q(21).decode()), ("TTTTGGGGCCCCAAAATTTTG", _q(21, b"#").decode())), (("NNN", "III"), ("ACG", "III"))])
    cs = b"ACGTACGTACGTACGTACGTACGTACGT" + b"NNNNNNNNNN" + b"GGGGCCCCAAAATTTTGGGGCCCC"
    cq = bytes(33 + (i * 5) % 60 for i in range(len(cs)))
    ex = b"TTTTTTTTTTTTTTTTTTTTTTGA" + b"NACGT"
    eq = bytes(40 + i % 40 for i in range(len(ex)))
    entries = [NR.single(1, 27), NR.single(28, 10), NR.single(0, 24, NR.SRC_BYTES), NR.single(5, 0),  # singles: kept, N, kept (merged read), empty
               NR.trivial(0), NR.trivial(1), NR.trivial(2, rev=True), NR.trivial(3, is_paired=True), NR.trivial(4, rev=True, is_paired=True),
               NR.trivial(3, rev=True, is_paired=True),
               NR.paired(0, 28, 38, 24), NR.paired(28, 10, 38, 24), NR.paired(3, 21, 0, 22, NR.SRC_CONSENSUS, NR.SRC_BYTES), NR.paired(0, 5, 7, 0)]
    got = _check(reads, (cs, cq), entries, (ex, eq))
    assert got.new_id.tolist() == [0, -1, 1, -1, 2, -1, 3, 4, -1, 5, 6, -1, 7, -1]
    assert got.counts["n_dropped_n_rate"] == 4 and got.counts["n_dropped_empty"] == 2 and got.counts["n_bad"] == 0
    assert got.reads.read_first_seq.tolist() == [0, 1, 2, 3, 4, 6, 8, 10, 12]


def test_restatement_every_bad_entry_case():
    reads = ReadSet.from_lists([("ACGTACGTACGTACGTACGTACG", _q(23).decode())], [(("ACGTACGTACGTACGTACGTA", _q(21).decode()), ("TTTTGGGGCCCCAAAATTTTG", _q(21).decode()))])
    cs, ex = b"ACGTACGTACGTACGTACGTACGTACGT", b"TTTTTTTTTTTTTTTTTTTTTTGA"
    bad = [NR.single(0, 29), NR.single(28, 1), NR.single(29, 0), NR.single(2 ** 63, 2 ** 31),     # ranges outside the consensus bytes
           NR.single(1, 24, NR.SRC_BYTES), NR.paired(0, 5, 20, 5, NR.SRC_CONSENSUS, NR.SRC_BYTES),  # ... and outside the extra bytes
           NR.single(0, 5, 2), NR.paired(0, 5, 5, 5, 0, 7),                                       # no such source
           (0, 0, 5, 0, 0, 4, 0, 0, 0), (0, 0, 5, 0, 0, 255, 0, 0, 0),                            # no such kind
           (0, 0, 5, 0, 0, NR.NEXT_SINGLE, 0, 0, 2), (0, 0, 0, 0, 0, NR.NEXT_TRIVIAL, 0, 0, 2),   # rev > 1
           NR.trivial(2), NR.trivial(2 ** 32 - 1),                                                # read index out of range
           NR.trivial(0, is_paired=True), NR.trivial(1)]                                          # a paired kind on a single read, and the reverse
    good = [NR.single(0, 28), NR.single(28, 0), NR.single(0, 24, NR.SRC_BYTES), NR.trivial(0), NR.trivial(1, is_paired=True)]
    got = _check(reads, (cs, _q(len(cs))), bad + good, (ex, _q(len(ex))))
    assert got.status.tolist() == [NR.NEXT_BAD_ENTRY] * len(bad) + [0, 1, 0, 0, 0]
    assert got.counts["n_bad"] == len(bad)
    # no store at all: every trivial is bad, nothing is read
    got = _check(None, (cs, _q(len(cs))), [NR.trivial(0), NR.single(0, 28)])
    assert got.status.tolist() == [NR.NEXT_BAD_ENTRY, 0]


def test_restatement_empty_result():
    for entries in ([], [NR.single(0, 0)], [NR.single(0, 4), NR.trivial(0)]):
        got = NR.host_next_reads(None, np.frombuffer(b"NNNN", np.uint8), np.frombuffer(b"IIII", np.uint8), np.array(entries, NR.NEXT_ENTRY_DTYPE))
        assert got.empty and got.reads is None and (got.new_id == -1).all() and got.counts["n_kept"] == 0
    assert got.status.tolist() == [NR.NEXT_DROPPED_N_RATE, NR.NEXT_BAD_ENTRY]


def test_restatement_random_batches():
    rng = np.random.default_rng(5)
    for it in range(20):
        n_s, n_p = int(rng.integers(0, 6)), int(rng.integers(0, 6))

        def rnd(n, p_n):
            return bytes(rng.choice(list(b"ACGTN"), n, p=[(1 - p_n) / 4] * 4 + [p_n]).astype(np.uint8)), bytes(rng.integers(33, 90, n).astype(np.uint8))

        reads = ReadSet.from_lists([rnd(int(rng.integers(1, 70)), rng.choice([0, 0.04, 0.08])) for _ in range(n_s)],
                                   [(rnd(int(rng.integers(1, 40)), 0.03), rnd(int(rng.integers(1, 40)), 0.03)) for _ in range(n_p)])
        cons, extra = rnd(int(rng.integers(0, 400)), 0.045), rnd(int(rng.integers(0, 200)), 0.045)
        entries = []
        for _ in range(40):
            k = int(rng.integers(0, 4))
            if k <= 1:
                m = []
                for _ in range(2):
                    s = int(rng.integers(0, 2))
                    room = len((cons, extra)[s][0])
                    off = int(rng.integers(0, room + 2))
                    m.append((off, int(rng.integers(0, max(1, room - off + (rng.random() < 0.1)) + 1)) if rng.random() < 0.9 else 0, s))
                entries.append(NR.single(m[0][0], m[0][1], m[0][2]) if k == 0 else NR.paired(m[0][0], m[0][1], m[1][0], m[1][1], m[0][2], m[1][2]))
            else:
                entries.append(NR.trivial(int(rng.integers(0, n_s + n_p + 1)), bool(rng.integers(0, 2)), k == 3))
        _check(reads, cons, entries, extra, keep_singletons=int(rng.integers(0, 50)))


PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "hcsr.h"
int main(void) {
    printf("entry %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hc_sr_next_entry), offsetof(hc_sr_next_entry, off1), offsetof(hc_sr_next_entry, off2),
           offsetof(hc_sr_next_entry, len1), offsetof(hc_sr_next_entry, len2), offsetof(hc_sr_next_entry, read), offsetof(hc_sr_next_entry, kind),
           offsetof(hc_sr_next_entry, src1), offsetof(hc_sr_next_entry, src2), offsetof(hc_sr_next_entry, rev));
    printf("settings %zu %zu\n", sizeof(hc_sr_next_settings), offsetof(hc_sr_next_settings, keep_singletons));
    printf("counts %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hc_sr_next_counts), offsetof(hc_sr_next_counts, n_kept),
           offsetof(hc_sr_next_counts, n_dropped_empty), offsetof(hc_sr_next_counts, n_dropped_n_rate), offsetof(hc_sr_next_counts, n_dropped_short),
           offsetof(hc_sr_next_counts, n_bad), offsetof(hc_sr_next_counts, n_seq), offsetof(hc_sr_next_counts, n_bytes),
           offsetof(hc_sr_next_counts, ms_device), offsetof(hc_sr_next_counts, ms_plan));
    printf("enum %d %d %d %d %d %d %d %d %d %d %d %d\n", HC_SR_NEXT_SINGLE, HC_SR_NEXT_PAIRED, HC_SR_NEXT_TRIVIAL, HC_SR_NEXT_TRIVIAL_PAIRED, HC_SR_SRC_CONSENSUS,
           HC_SR_SRC_BYTES, HC_SR_NEXT_KEPT, HC_SR_NEXT_DROPPED_EMPTY, HC_SR_NEXT_DROPPED_N_RATE, HC_SR_NEXT_DROPPED_SHORT, HC_SR_NEXT_BAD_ENTRY, HC_SR_NEXT_EMPTY);
    /* one read "ACGTN" reversed, one consensus super-read */
    const uint8_t bases[] = "AACGTTTTTTTTTTTTTTTTTTTTN", quals[] = "ABCDEFGHIJKLMNOPQRSTUVWXY";
    const uint64_t seq_off[2] = {0, 25};
    const uint32_t first[2] = {0, 1};
    const uint8_t cs[] = "GGGG", cq[] = "5555";
    hc_sr_next_entry e[2];
    memset(e, 0, sizeof e);
    e[0].len1 = 4; e[0].kind = HC_SR_NEXT_SINGLE;
    e[1].kind = HC_SR_NEXT_TRIVIAL; e[1].rev = 1;
    hc_sr_next_settings st = {0, 0};
    int32_t id[2]; uint32_t status[2]; hc_sr_next_counts cn; uint64_t nb = 0, off[5]; uint32_t of[3]; uint8_t ob[32], oq[32];
    int rc = hc_host_sr_next_reads(bases, quals, seq_off, first, 1, cs, cq, 4, e, 2, NULL, NULL, 0, &st, id, status, &cn, NULL, NULL, 0, &nb, off, of);
    if (rc != HC_ERR_ARG || nb != 29) return 3; /* count first ... */
    rc = hc_host_sr_next_reads(bases, quals, seq_off, first, 1, cs, cq, 4, e, 2, NULL, NULL, 0, &st, id, status, &cn, ob, oq, sizeof ob, &nb, off, of);
    if (rc != HC_OK || id[0] != 0 || id[1] != 1 || cn.n_kept != 2 || off[1] != 4 || off[2] != 29 || of[2] != 2) return 4; /* ... then fetch */
    printf("bytes %.*s %.*s\n", 29, (const char*)ob, 29, (const char*)oq);
    return 0;
}
'''


def test_next_reads_header_is_c99_and_calls_through(tmp_path):
    src = tmp_path / "abi_srnext.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_srnext")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    d = NR.NEXT_ENTRY_DTYPE
    assert out["entry"] == "32 " + " ".join(str(d.fields[k][1]) for k in ("off1", "off2", "len1", "len2", "read", "kind", "src1", "src2", "rev"))
    assert out["settings"] == f"{C.sizeof(N.hc_sr_next_settings)} {N.hc_sr_next_settings.keep_singletons.offset}" == "8 0"
    t = N.hc_sr_next_counts
    assert out["counts"] == f"{C.sizeof(t)} " + " ".join(str(getattr(t, k).offset) for k, _ in t._fields_) and C.sizeof(t) == 72
    assert out["enum"] == " ".join(str(v) for v in (NR.NEXT_SINGLE, NR.NEXT_PAIRED, NR.NEXT_TRIVIAL, NR.NEXT_TRIVIAL_PAIRED, NR.SRC_CONSENSUS, NR.SRC_BYTES,
                                                    NR.NEXT_KEPT, NR.NEXT_DROPPED_EMPTY, NR.NEXT_DROPPED_N_RATE, NR.NEXT_DROPPED_SHORT, NR.NEXT_BAD_ENTRY,
                                                    NR.NEXT_EMPTY))
    assert out["bytes"] == "GGGGNAAAAAAAAAAAAAAAAAAAACGTT 5555YXWVUTSRQPONMLKJIHGFEDCBA"


def test_entry_points_exist_and_cite_the_reference():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in ("hc_sr_keep_device", "hc_sr_set_next_reads", "hc_sr_next_reads_fetch", "hc_host_sr_next_reads"):
        assert name in src and hasattr(N.lib, name)
    for cite in ("SRBuilder.cpp:983", "Read.h:203-234", "1278-1380", ":1416-1556", "subreads.txt"):
        assert cite in src
    assert N.lib.hc_sr_set_next_reads(None, None, 0, None, None, 0, None, None, None, None) == -1  # HC_ERR_ARG
    assert N.lib.hc_sr_keep_device(None, 1) == -1
