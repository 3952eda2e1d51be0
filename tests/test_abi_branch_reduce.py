"""The hc_br_reduce calls and hc_host_br_reduce in include/hcsr.h as C99: the header compiles in a plain C program that names the new structures,
their sizes and offsets are the ones the Python structures and dtypes assume, the symbols are exported, the section sits behind the evidence
section, cites the reference and says what pins the result to a standard library, and the calls answer NULL arguments with HC_ERR_ARG (no GPU
is touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import branch_evidence as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_host_br_parse_thresholds", "hc_br_reduce", "hc_br_reduce_fetch", "hc_host_br_reduce", "hc_host_br_map_order")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
int main(void) {
    hc_br_threshold th;
    hc_br_reduce_settings st;
    hc_br_reduce_counts cn;
    hc_br_reduce_tables t;
    hc_br_host_graph_out g;
    hc_br_component c;
    uint64_t n = 0;
    printf("sizes %lu %lu %lu %lu %lu %lu\n", (unsigned long)sizeof th, (unsigned long)sizeof st, (unsigned long)sizeof cn, (unsigned long)sizeof t,
           (unsigned long)sizeof g, (unsigned long)sizeof c);
    printf("component %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_br_component, dist), (unsigned long)offsetof(hc_br_component, min_evidence),
           (unsigned long)offsetof(hc_br_component, outcome), (unsigned long)offsetof(hc_br_component, host_finished),
           (unsigned long)offsetof(hc_br_component, edge_first), (unsigned long)offsetof(hc_br_component, edge_count));
    printf("settings %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_br_reduce_settings, careful), (unsigned long)offsetof(hc_br_reduce_settings, diploid),
           (unsigned long)offsetof(hc_br_reduce_settings, verbose), (unsigned long)offsetof(hc_br_reduce_settings, thresholds),
           (unsigned long)offsetof(hc_br_reduce_settings, n_thresholds));
    printf("counts %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_br_reduce_counts, n_components), (unsigned long)offsetof(hc_br_reduce_counts, n_host_finished),
           (unsigned long)offsetof(hc_br_reduce_counts, ms_device), (unsigned long)offsetof(hc_br_reduce_counts, ms_copy));
    printf("enums %d %d %d %d %d %d %d\n", HC_BR_RED_KEPT, HC_BR_RED_NOT_KEPT, HC_BR_RED_NO_THRESHOLD, HC_BR_RED_CAREFUL, HC_BR_RED_HOST_NO_ROW,
           HC_BR_RED_HOST_SHARED_EDGE, HC_BR_RED_HOST_DIPLOID);
    printf("rc %d %d %d %d %d\n", hc_host_br_parse_thresholds(NULL, 3, &th, 1, &n, NULL), hc_br_reduce(NULL, &st, &cn), hc_br_reduce_fetch(NULL, &t),
           hc_host_br_reduce(NULL, NULL, &st, &cn, &t, &g), hc_host_br_map_order(3, NULL));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layout_python_assumes(tmp_path):
    src = tmp_path / "abi_branch_reduce.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_branch_reduce")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    assert out["sizes"] == (f"{C.sizeof(N.hc_br_threshold)} {C.sizeof(N.hc_br_reduce_settings)} {C.sizeof(N.hc_br_reduce_counts)} "
                            f"{C.sizeof(N.hc_br_reduce_tables)} {C.sizeof(N.hc_br_host_graph_out)} {BR.COMPONENT_DTYPE.itemsize}") == "8 32 120 56 72 32"
    assert BR.THRESHOLD_DTYPE.itemsize == 8
    f = BR.COMPONENT_DTYPE.fields
    assert out["component"] == " ".join(str(f[k][1]) for k in ("dist", "min_evidence", "outcome", "host_finished", "edge_first", "edge_count")) == "0 4 8 12 16 24"
    s = N.hc_br_reduce_settings
    assert out["settings"] == f"{s.careful.offset} {s.diploid.offset} {s.verbose.offset} {s.thresholds.offset} {s.n_thresholds.offset}" == "0 4 8 16 24"
    c = N.hc_br_reduce_counts
    assert out["counts"] == f"{c.n_components.offset} {c.n_host_finished.offset} {c.ms_device.offset} {c.ms_copy.offset}" == "0 72 80 96"
    assert out["enums"] == (f"{BR.RED_KEPT} {BR.RED_NOT_KEPT} {BR.RED_NO_THRESHOLD} {BR.RED_CAREFUL} {BR.RED_HOST_NO_ROW} {BR.RED_HOST_SHARED_EDGE} "
                            f"{BR.RED_HOST_DIPLOID}") == "0 1 2 3 1 2 4"
    assert out["rc"] == " ".join(["-1"] * 5)  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    st, cn, t = N.hc_br_reduce_settings(), N.hc_br_reduce_counts(), N.hc_br_reduce_tables()
    assert N.lib.hc_br_reduce(None, C.byref(st), C.byref(cn)) == -1
    assert N.lib.hc_br_reduce_fetch(None, C.byref(t)) == -1
    assert N.lib.hc_host_br_reduce(None, None, C.byref(st), C.byref(cn), None, None) == -1
    n = C.c_uint64(7)
    assert N.lib.hc_host_br_parse_thresholds(None, 0, None, 0, C.byref(n), None) == 0 and n.value == 0  # an empty text: an empty table
    assert N.lib.hc_host_br_parse_thresholds(b"1\t2\t3\n", 6, None, 0, C.byref(n), None) == -1 and n.value == 1  # count, then fetch


def test_comments_cite_the_reference_and_say_what_pins_the_result():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        assert re.search(r"\*/\s*int " + name + r"\(", src), name + ": no comment in front of the declaration"
    start = src.index("the reduction: the second half of BranchReduction::readBasedBranchReduction")
    assert src.index("read evidence for branching edges: the first half") < start < src.index("singles.fastq, paired1.fastq, paired2.fastq and")
    section = src[start:src.index("singles.fastq, paired1.fastq, paired2.fastq and")]
    for cite in (":82-227", ":745-1272", ":753-781", ":806-833", ":163-204", ":1100-1122", ":1053-1096", ":849-855", ":928-932", ":172-177", ":206-207",
                 ":1164", ":1088", ":1029-1031", "src/OverlapGraph.cpp:104-147", ":134-155", ":157", ":193-201", ":83-85", ":217-225", ":219-222", ":1252-1257",
                 ":137-155", "std::stoi", "libstdc++", "recorded again", "FIRST record", "FIRST entry", "adj_in", "target order", "HC_ERR_STATE", "HC_ERR_ARG",
                 "count, then fetch", "A fixed number of launches", "hc_graph_merge_pairs", "hc_fno1_run", "spent"):
        assert cite in section, cite
    # the evidence section no longer leaves the second half to the caller
    first_half = src[src.index("read evidence for branching edges: the first half"):start]
    assert "it stays with the caller" not in first_half and "hc_br_reduce" in first_half
