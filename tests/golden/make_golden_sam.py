#!/usr/bin/env python3
"""Golden vectors for the SAM ingest: bwa's SAM records -> SAVAGE's 13-column overlaps file, as the reference's
scripts/sam2overlaps.py does it (savage.py --ref, polyte.py's reference-guided start).

The reference script is Python 2 and is translated IN MEMORY by lib2to3, exactly as make_golden_sfo.py does it (nothing of it is
written to disk).  Two shims: `round` is bound to Python 2's round-half-away-from-zero, which the script relies on for the overlap
percentage (sam2overlaps.py:333), and `time.clock`, which the script imports and Python 3.10 lacks, gets a stand-in while the
module is loaded.  Per case tests/golden/sam/cases.json records the three input texts, min_overlap_len and either the output file's
bytes or the type of the exception the script died of.  Data only.

The maker asserts, from the script's output alone (and the ids it gave the inputs), that the set covers what the ingest has to get
right; see check_coverage.  One thing the script has cannot be reached by any input: `assert perc <= 100` (:338) — the overlap
length is min(len2 - pos, len1) with pos >= 0, never above the shorter read."""
import io
import json
import math
import os
import random
import sys
import tempfile
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sam")
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/scripts/sam2overlaps.py"


def py2_round(x):
    """Python 2's round(): nearest integer as a float, halves away from zero (C round())."""
    f = math.floor(abs(x))
    r = f + 1.0 if abs(x) - f >= 0.5 else float(f)
    return r if x >= 0 else -r


def load_reference_module():
    warnings.filterwarnings("ignore")
    from lib2to3 import refactor

    rt = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    code = str(rt.refactor_string(open(REF).read(), "sam2overlaps.py"))
    ns = {"__name__": "sam2overlaps_ref", "round": py2_round}
    had = hasattr(time, "clock")
    if not had:
        time.clock = time.perf_counter
    try:
        exec(compile(code, REF, "exec"), ns)
    finally:
        if not had:
            del time.clock
    return ns


def run_reference(ns, sam_s, sam_p, ref, min_overlap_len):
    """-> (output bytes, None) or (None, exception type name)"""
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for name, text in (("s.sam", sam_s), ("p.sam", sam_p), ("ref.fasta", ref)):
            paths[name] = os.path.join(d, name)
            with open(paths[name], "w", newline="") as f:
                f.write(text)
        out = os.path.join(d, "out.txt")
        argv, stdout = sys.argv, sys.stdout
        sys.argv = ["sam2overlaps.py", "--ref", paths["ref.fasta"], "--out", out, "--min_overlap_len", str(min_overlap_len)]
        if sam_s is not None and sam_s != "":
            sys.argv += ["--sam_s", paths["s.sam"]]
        if sam_p is not None and sam_p != "":
            sys.argv += ["--sam_p", paths["p.sam"]]
        sys.stdout = io.StringIO()
        try:
            ns["main"]()
        except BaseException as e:  # SystemExit included
            return None, type(e).__name__
        finally:
            sys.argv, sys.stdout = argv, stdout
        return (open(out).read() if os.path.exists(out) else ""), None


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def aln(rid, flag, ref, pos, cigar, seqlen):
    return "\t".join([str(rid), str(flag), ref, str(pos), "60", cigar, "=", "0", "0", "A" * seqlen, "I" * seqlen])


def fasta(*refs):
    return "".join(">%s description\n%s\n" % (name, "\n".join("ACGT" * (n // 4) + "A" * (n % 4) for n in [length])) for name, length in refs)


HEADER = "@HD\tVN:1.0\n@SQ\tSN:r1\tLN:1000\n"


def random_cigar(rng, n):
    """all M, or clips and an indel between matches (about n query bases: the SEQ written is as long as the CIGAR says, seq_len)"""
    if rng.random() < 0.5:
        return "%dM" % n
    a, b = rng.randrange(3, n // 2), rng.randrange(1, 4)
    return rng.choice(("", "", "%dS" % b, "%dH" % b)) + "%dM%d%s%dM" % (a, b, rng.choice("ID"), n - a - b) + rng.choice(("", "", "2H"))


def seq_len(cigar):
    import re

    return sum(int(k) for k, c in re.findall(r"(\d+)([A-Z=])", cigar) if c in "MIS=X")


def random_case(seed, n_single, n_pair, refs, min_overlap_len, lens=(100,), span=600):
    rng = random.Random(seed)
    names = [r[0] for r in refs]
    s, p = [HEADER.rstrip("\n")], [HEADER.rstrip("\n")]
    for k in range(n_single):
        cg = random_cigar(rng, rng.choice(lens))
        flag = rng.choice((0, 16, 0, 4))
        s.append(aln(k, flag, rng.choice(names), rng.randrange(1, span), cg if flag != 4 else "*", seq_len(cg)))
    for k in range(n_pair):
        c1, c2 = random_cigar(rng, rng.choice(lens)), random_cigar(rng, rng.choice(lens))
        a = rng.randrange(1, span)
        b = a + rng.randrange(0, 90)
        ref = rng.choice(names)
        kind = rng.random()
        if kind < 0.55:
            f1, f2, p1, p2 = 65, 129, a, b
        elif kind < 0.85:
            f1, f2, p1, p2 = 81, 145, b, a
        elif kind < 0.92:
            f1, f2, p1, p2 = 65, 145, a, b  # discarded
        else:
            f1, f2, p1, p2 = 77, 141, a, b  # unmapped
        rid = 1000 + k
        p.append(aln(rid, f1, ref, p1, c1 if f1 != 77 else "*", seq_len(c1)))
        if rng.random() < 0.04:
            continue  # a mate is missing: the id mismatch of :241
        p.append(aln(rid, f2, ref, p2, c2 if f2 != 141 else "*", seq_len(c2)))
    return dict(sam_s="\n".join(s) + "\n", sam_p="\n".join(p) + "\n", ref=fasta(*refs), min_overlap_len=min_overlap_len)


def crafted():
    C = {}
    ref1 = fasta(("r1", 400))
    # length == min_overlap_len is not written, min_overlap_len + 1 is
    C["strict_length"] = dict(sam_s="\n".join([aln(1, 0, "r1", 100, "100M", 100), aln(2, 0, "r1", 149, "100M", 100), aln(3, 0, "r1", 150, "100M", 100)]) + "\n",
                              sam_p="", ref=ref1, min_overlap_len=50)
    # a read stays active at exactly len - d == min_overlap_len (r1) and leaves at one less (r2); the third read's corrected overlap is
    # long enough either way because of the deletion in the first
    keep = [aln(1, 0, "r1", 100, "50M10D50M", 100), aln(11, 0, "r2", 100, "50M10D50M", 100), aln(2, 0, "r1", 150, "100M", 100),
            aln(12, 0, "r2", 151, "100M", 100), aln(3, 0, "r1", 151, "100M", 100), aln(13, 0, "r2", 152, "100M", 100)]
    C["active_boundary"] = dict(sam_s="\n".join(keep) + "\n", sam_p="", ref=fasta(("r1", 400), ("r2", 400)), min_overlap_len=50)
    # a pair of reads rejected for a negative corrected position (a long deletion at the front read's start)
    C["negative_position"] = dict(sam_s="\n".join([aln(1, 0, "r1", 100, "10M60D90M", 100), aln(2, 0, "r1", 120, "100M", 100), aln(3, 16, "r1", 130, "100M", 100)]) + "\n",
                                  sam_p="", ref=ref1, min_overlap_len=0)
    # single record / paired read: overlap_pos2 < 0 is skipped (single 4), >= 0 is not (single 3); a single and a pair tied at 100
    pairs = [aln(1000, 65, "r1", 100, "100M", 100), aln(1000, 129, "r1", 130, "100M", 100)]
    C["second_mate_behind"] = dict(sam_s="\n".join([aln(1, 0, "r1", 100, "100M", 100), aln(3, 0, "r1", 125, "100M", 100), aln(4, 0, "r1", 140, "100M", 100)]) + "\n",
                                   sam_p="\n".join(pairs) + "\n", ref=ref1, min_overlap_len=10)
    # the paired file's state machine: normal, reverse, discarded, an id mismatch, unmapped lines; ord 1 and 2
    pp = [aln(1000, 65, "r1", 100, "100M", 100), aln(1000, 129, "r1", 300, "100M", 100),  # normal
          aln(1001, 77, "*", 0, "*", 100), aln(1001, 141, "*", 0, "*", 100),                # unmapped
          aln(1002, 81, "r1", 340, "100M", 100), aln(1002, 145, "r1", 120, "100M", 100),  # reverse: stored [second, first]
          aln(1003, 65, "r1", 130, "100M", 100), aln(1003, 145, "r1", 330, "100M", 100),  # discarded
          aln(1004, 65, "r1", 135, "100M", 100),                                           # its mate is missing ...
          aln(1005, 65, "r1", 140, "100M", 100), aln(1005, 129, "r1", 290, "100M", 100),  # ... ord 2 against 1000 (second mate in front)
          aln(1006, 65, "r1", 150, "3S97M", 100), aln(1006, 129, "r1", 350, "95M5H", 95)]
    C["paired_machine"] = dict(sam_s=HEADER + aln(5, 4, "*", 0, "*", 50) + "\n", sam_p=HEADER + "\n".join(pp) + "\n", ref=ref1, min_overlap_len=20)
    # clips and indels, one and nine operations
    cg = [aln(1, 0, "r1", 100, "5S95M", 100), aln(2, 0, "r1", 110, "5H95M", 95), aln(3, 16, "r1", 120, "90M10H", 90), aln(4, 0, "r1", 130, "40M3I57M", 100),
          aln(5, 0, "r1", 140, "40M3D60M", 100), aln(6, 0, "r1", 150, "2S10M1I20M2D30M1I30M4S2H", 98), aln(7, 0, "r1", 155, "100M", 100)]
    C["clips_and_indels"] = dict(sam_s="\n".join(cg) + "\n", sam_p="", ref=ref1, min_overlap_len=30)
    # past the reference's end: the record at 310 is still processed (the loop tests the previous position), the one at 320 is not
    C["reference_end"] = dict(sam_s="\n".join([aln(1, 0, "r1", 100, "100M", 100), aln(2, 0, "r1", 250, "100M", 100), aln(3, 0, "r1", 310, "100M", 100),
                                               aln(4, 0, "r1", 320, "100M", 100)]) + "\n", sam_p="", ref=fasta(("r1", 300)), min_overlap_len=10)
    C["first_past_end"] = dict(sam_s="\n".join([aln(1, 0, "r1", 300, "100M", 100), aln(2, 0, "r1", 310, "100M", 100)]) + "\n", sam_p="", ref=fasta(("r1", 300)),
                               min_overlap_len=10)
    # 1 / 200 * 100 = 0.5 -> 1 under Python 2's round
    C["half_percent"] = dict(sam_s="\n".join([aln(1, 0, "r1", 100, "200M", 200), aln(2, 0, "r1", 299, "200M", 200)]) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    # ids that are not numbers, a FASTA over several lines with a sequence line in front of the first header
    C["text_ids"] = dict(sam_s="\n".join([aln("read/a", 0, "r1", 100, "100M", 100), aln("0012", 16, "r1", 120, "100M", 100), aln("x y", 0, "r1", 130, "100M", 100)]) + "\n",
                         sam_p="", ref="ACGT\n>r0\n>r1 one\nACGTACGT\n" + "ACGT" * 100 + "\n", min_overlap_len=5)
    # ---- where the script dies ----
    ok = aln(1, 0, "r1", 100, "100M", 100)
    C["err_star_cigar"] = dict(sam_s=ok + "\n" + aln(2, 0, "r1", 120, "*", 100) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    C["err_unknown_reference"] = dict(sam_s=ok + "\n" + aln(2, 0, "r9", 120, "100M", 100) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    C["err_short_line"] = dict(sam_s=ok + "\n" + "\t".join(aln(2, 0, "r1", 120, "100M", 100).split("\t")[:10]) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    C["err_not_a_number"] = dict(sam_s=ok + "\n" + aln(2, 0, "r1", "12x", "100M", 100) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    C["err_flag_not_a_number"] = dict(sam_s="", sam_p=aln(2, "0x10", "r1", 120, "100M", 100) + "\n", ref=ref1, min_overlap_len=0)
    C["err_cigar_without_count"] = dict(sam_s=ok + "\n" + aln(2, 0, "r1", 120, "M100", 100) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    # a SEQ shorter than its CIGAR: the second overlap's length is negative, `assert perc >= 0` (:334)
    C["err_perc_assert"] = dict(sam_s=aln(1, 0, "r1", 100, "100M", 10) + "\n",
                                sam_p=aln(1000, 65, "r1", 101, "100M", 100) + "\n" + aln(1000, 129, "r1", 160, "100M", 100) + "\n", ref=ref1, min_overlap_len=0)
    # an empty SEQ in a second mate: min(len1, len2) == 0 (:333)
    C["err_zero_length"] = dict(sam_s=aln(1, 0, "r1", 100, "100M", 100) + "\n",
                                sam_p=aln(1000, 65, "r1", 101, "100M", 100) + "\n" + aln(1000, 129, "r1", 160, "100M", 0) + "\n", ref=ref1, min_overlap_len=0)
    C["err_empty_fasta"] = dict(sam_s=ok + "\n", sam_p="", ref="", min_overlap_len=0)
    C["err_fasta_without_sequence"] = dict(sam_s=ok + "\n", sam_p="", ref=">r1\n", min_overlap_len=0)
    C["err_no_aligned_read"] = dict(sam_s=HEADER + aln(1, 4, "*", 0, "*", 100) + "\n", sam_p="", ref=ref1, min_overlap_len=0)
    return C


def cases():
    C = crafted()
    two = (("r1", 260), ("r2", 240))
    C["random_mixed"] = random_case(4, 22, 18, two, 20, lens=(30, 40, 60, 90), span=90)  # two references interleaved, mixed lengths
    C["random_min_overlap_0"] = random_case(5, 10, 8, (("r1", 100),), 0, lens=(30, 40), span=120)
    return C


# ---- what the set has to contain ------------------------------------------------------------------------------------------------
def lines_of(case):
    return [ln.split("\t") for ln in case["expected"].splitlines()]


def has(case, id1, id2):
    return any(f[0] == str(id1) and f[1] == str(id2) for f in lines_of(case))


def check_coverage(C):
    paired = lambda x: x.isdigit() and int(x) >= 1000  # the makers' own id ranges
    branches, ords = set(), set()
    for c in C.values():
        if "expected" not in c:
            continue
        for f in lines_of(c):
            assert len(f) == 13
            ords.add(f[4])
            if f[11] == "s" and f[12] == "s":
                assert f[3] == f[8] == f[10] == "0" and f[4] == "-"
                branches.add("ss")
            elif f[11] == "p":
                branches.add("pp")
            else:  # the script writes s, p for both mixed branches (:416, :438)
                branches.add("sp" if paired(f[0]) else "ps")
    assert branches == {"ss", "ps", "sp", "pp"}, branches
    assert {"1", "2", "-"} <= ords, ords
    c = C["strict_length"]
    assert has(c, 1, 2) and not has(c, 1, 3) and has(c, 2, 3)
    assert [f[9] for f in lines_of(c) if f[:2] == ["1", "2"]] == ["51"]
    c = C["active_boundary"]
    assert has(c, 1, 3) and not has(c, 11, 13) and has(c, 12, 13)
    assert not has(C["negative_position"], 1, 2) and has(C["negative_position"], 2, 3)
    c = C["second_mate_behind"]
    assert has(c, 1000, 3) and not has(c, 1000, 4) and has(c, 1, 1000) and not has(c, 1000, 1)  # the tie: the single is first
    c = C["paired_machine"]
    ids = {f[0] for f in lines_of(c)} | {f[1] for f in lines_of(c)}
    assert "1000" in ids and "1002" in ids and "1005" in ids and "1003" not in ids and "1004" not in ids and "1001" not in ids
    assert any(f[6] == "-" for f in lines_of(c) if f[1] == "1002") and any(f[4] == "2" for f in lines_of(c))
    assert len(lines_of(C["clips_and_indels"])) >= 10
    c = C["reference_end"]
    assert has(c, 2, 3) and not has(c, 3, 4)
    assert C["first_past_end"]["expected"] == ""
    assert [f[7] for f in lines_of(C["half_percent"])] == ["1"]
    assert has(C["text_ids"], "read/a", "0012")
    assert len(C["random_min_overlap_0"]["expected"]) > 0 and C["random_min_overlap_0"]["min_overlap_len"] == 0
    assert len(lines_of(C["random_mixed"])) > 40
    want = {"err_star_cigar": "IndexError", "err_unknown_reference": "KeyError", "err_short_line": "ValueError", "err_not_a_number": "ValueError",
            "err_flag_not_a_number": "ValueError", "err_cigar_without_count": "ValueError", "err_perc_assert": "AssertionError",
            "err_zero_length": "ZeroDivisionError", "err_empty_fasta": "SystemExit", "err_fasta_without_sequence": "SystemExit",
            "err_no_aligned_read": "SystemExit"}
    for name, err in want.items():
        assert C[name].get("error") == err, (name, C[name].get("error"))
    assert all(("error" in c) == name.startswith("err_") for name, c in C.items())


def main():
    ns = load_reference_module()
    C = cases()
    for name, c in C.items():
        out, err = run_reference(ns, c["sam_s"], c["sam_p"], c["ref"], c["min_overlap_len"])
        if err is None:
            c["expected"] = out
        else:
            c["error"] = err
        print(name, err if err else "%d lines" % out.count("\n"))
    check_coverage(C)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(C[k], sort_keys=True, separators=(",", ":")) for k in sorted(C)) + "\n}\n")  # a case a line
    print("wrote", os.path.getsize(os.path.join(OUT, "cases.json")), "bytes")


if __name__ == "__main__":
    main()
