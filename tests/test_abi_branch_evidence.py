"""The hc_br_* calls and hc_host_br_evidence in include/hcsr.h as C99: the header compiles in a plain C program that names the structures, the
layouts are the ones the Python structures and dtypes assume, the symbols are exported, the section sits behind the originals section and in
front of the FASTQ section, cites the reference and restates its quirks, and the calls answer NULL arguments with HC_ERR_ARG (no GPU is
touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import branch_evidence as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_br_set_original_reads", "hc_br_evidence", "hc_br_evidence_fetch", "hc_host_br_evidence")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
int main(void) {
    hc_br_settings st;
    hc_br_counts cn;
    hc_br_tables t;
    hc_br_host_input in;
    hc_br_branch b;
    printf("sizes %lu %lu %lu %lu %lu\n", (unsigned long)sizeof st, (unsigned long)sizeof cn, (unsigned long)sizeof t, (unsigned long)sizeof in,
           (unsigned long)sizeof b);
    printf("branch %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_br_branch, node), (unsigned long)offsetof(hc_br_branch, side),
           (unsigned long)offsetof(hc_br_branch, status), (unsigned long)offsetof(hc_br_branch, is_false), (unsigned long)offsetof(hc_br_branch, dist),
           (unsigned long)offsetof(hc_br_branch, nb_count), (unsigned long)offsetof(hc_br_branch, nb_first), (unsigned long)offsetof(hc_br_branch, diff_first),
           (unsigned long)offsetof(hc_br_branch, diff_count), (unsigned long)offsetof(hc_br_branch, n_neighbours));
    printf("settings %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_br_settings, se_count), (unsigned long)offsetof(hc_br_settings, pe_count),
           (unsigned long)offsetof(hc_br_settings, original_readcount), (unsigned long)offsetof(hc_br_settings, min_overlap_len),
           (unsigned long)offsetof(hc_br_settings, edge_threshold));
    printf("enums %d %d %d %d %d %d %d %d %u\n", HC_BR_IN, HC_BR_OUT, HC_BR_OK, HC_BR_PAIRED_NEIGHBOUR, HC_BR_REPEATED_NEIGHBOUR, HC_BR_BAD_GEOMETRY,
           HC_BR_BAD_ORIGINAL, HC_BR_SOME_FAILED, HC_BR_MAX_DIFFS);
    printf("rc %d %d %d %d\n", hc_br_set_original_reads(NULL, NULL, NULL, 0), hc_br_evidence(NULL, NULL, NULL, 0, NULL, &cn), hc_br_evidence_fetch(NULL, &t),
           hc_host_br_evidence(NULL, &st, &cn, NULL, 1));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layout_python_assumes(tmp_path):
    src = tmp_path / "abi_branch_evidence.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_branch_evidence")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    assert out["sizes"] == (f"{C.sizeof(BR.hc_br_settings)} {C.sizeof(BR.hc_br_counts)} {C.sizeof(BR.hc_br_tables)} {C.sizeof(BR.hc_br_host_input)} "
                            f"{BR.BRANCH_DTYPE.itemsize}") == "40 72 104 128 40"
    f = BR.BRANCH_DTYPE.fields
    assert out["branch"] == " ".join(str(f[k][1]) for k in ("node", "side", "status", "is_false", "dist", "nb_count", "nb_first", "diff_first", "diff_count",
                                                               "n_neighbours")) == "0 4 5 6 8 12 16 24 32 36"
    s = BR.hc_br_settings
    assert out["settings"] == f"{s.se_count.offset} {s.pe_count.offset} {s.original_readcount.offset} {s.min_overlap_len.offset} {s.edge_threshold.offset}"
    assert out["enums"] == (f"{BR.BR_IN} {BR.BR_OUT} {BR.BR_OK} {BR.BR_PAIRED_NEIGHBOUR} {BR.BR_REPEATED_NEIGHBOUR} {BR.BR_BAD_GEOMETRY} {BR.BR_BAD_ORIGINAL} "
                            f"{BR.SOME_FAILED} {BR.MAX_DIFFS}") == "0 1 0 1 2 3 4 1 100"
    assert out["rc"] == " ".join(["-1"] * 4)  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    cn, t, st = BR.hc_br_counts(), BR.hc_br_tables(), BR.settings(0, 0, 0, 0, 0.0)
    assert N.lib.hc_br_set_original_reads(None, None, None, 0) == -1
    assert N.lib.hc_br_evidence(None, None, None, 0, C.byref(st), C.byref(cn)) == -1
    assert N.lib.hc_br_evidence_fetch(None, C.byref(t)) == -1
    assert N.lib.hc_host_br_evidence(None, C.byref(st), C.byref(cn), None, 1) == -1
    inp = BR.hc_br_host_input()
    assert N.lib.hc_host_br_evidence(C.byref(inp), C.byref(st), C.byref(cn), None, 1) == -1  # null offsets
    assert N.lib.hc_host_br_evidence(C.byref(inp), C.byref(st), None, None, 1) == -1          # nowhere to put the counts


def test_comments_cite_the_reference_and_restate_its_quirks():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        assert re.search(r"\*/\s*int " + name + r"\(", src), name + ": no comment in front of the declaration"
    start = src.index("read evidence for branching edges: the first half of BranchReduction::readBasedBranchReduction")
    assert src.index("the original-read index maps on the device, and subreads.txt") < start < src.index("singles.fastq, paired1.fastq, paired2.fastq and")
    section = src[start:src.index("singles.fastq, paired1.fastq, paired2.fastq and")]
    for cite in (":229-743", ":60-80", ":745-1272", ":414", ":556", ":627", ":304-321", ":318", ":720", ":449", ":521-530", ":675-684", ":330-332", ":349",
                 ":733-737", "src/Edge.h:41-56", ":412", ":554", ":446", ":471", ":625", ":605", ":616", ":300", ":319", ":328-335", ":367-384", ":476-511",
                 "src/ViralQuasispecies.cpp:341", "src/GraphAlgos.cpp:831", "vertex_read[v]", "count, then fetch", "HC_ERR_STATE", "HC_ERR_ARG", "--careful",
                 "target order", "A fixed number of launches", "contributes nothing"):
        assert cite in section, cite
    # the originals section no longer leaves BranchReduction to the caller
    before = src[:start]
    assert not re.search(r"Left to the caller:[^.]*BranchReduction", before)
    assert "hc_br_evidence" in before
