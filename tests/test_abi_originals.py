"""The hc_sr_originals_* calls and their host mirrors in include/hcsr.h as C99: the header compiles in a plain C program that calls the nine
calls and fills the structures, the layouts are the ones the Python structures and the numpy dtype assume, the symbols are exported, the
comments cite the reference and state the order contract, and the calls answer NULL arguments with an error (no GPU is touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import originals as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_sr_originals_init", "hc_sr_originals_load", "hc_sr_originals_fetch", "hc_sr_originals_next", "hc_sr_originals_write_text",
         "hc_sr_originals_text_fetch", "hc_host_sr_originals_next", "hc_host_sr_originals_text", "hc_host_sr_originals_parse")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
int main(void) {
    hc_sr_original o = {7, -1, 2, 100, 90, 1, 1, {0, 0}};
    hc_sr_originals_input in;
    hc_sr_originals_output out;
    hc_sr_originals_text_counts cn;
    uint64_t n = 0;
    int status[4] = {HC_SR_ORIG_OK, HC_SR_ORIG_EMPTY_SOURCE, HC_SR_ORIG_SEQ0_OF_PAIRED, HC_SR_ORIG_RANGE};
    printf("sizes %lu %lu %lu %lu\n", (unsigned long)sizeof o, (unsigned long)sizeof in, (unsigned long)sizeof out, (unsigned long)sizeof cn);
    printf("entry %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_sr_original, id), (unsigned long)offsetof(hc_sr_original, index1),
           (unsigned long)offsetof(hc_sr_original, index2), (unsigned long)offsetof(hc_sr_original, len1), (unsigned long)offsetof(hc_sr_original, len2),
           (unsigned long)offsetof(hc_sr_original, paired), (unsigned long)offsetof(hc_sr_original, forward));
    printf("offsets %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_sr_originals_input, n_cliques), (unsigned long)offsetof(hc_sr_originals_input, n_srs),
           (unsigned long)offsetof(hc_sr_originals_input, n_vertices), (unsigned long)offsetof(hc_sr_originals_input, new_read_count),
           (unsigned long)offsetof(hc_sr_originals_input, first_it), (unsigned long)offsetof(hc_sr_originals_output, n_entries),
           (unsigned long)offsetof(hc_sr_originals_output, ms_copy));
    printf("status %d %d %d %d %d\n", status[0], status[1], status[2], status[3], HC_SR_ORIG_SOME_FAILED);
    printf("rc %d %d %d %d %d %d %d %d %d\n", hc_sr_originals_init(NULL), hc_sr_originals_load(NULL, NULL, &o, 0),
           hc_sr_originals_fetch(NULL, NULL, 0, NULL, 0, &n, &n), hc_sr_originals_next(NULL, &in, &out), hc_sr_originals_write_text(NULL, &cn),
           hc_sr_originals_text_fetch(NULL, 0, 0, NULL), hc_host_sr_originals_next(NULL, NULL, 0, NULL, NULL, NULL, 0, 1),
           hc_host_sr_originals_text(NULL, NULL, 0, NULL, 0, NULL), hc_host_sr_originals_parse(NULL, 5, NULL, 0, NULL, 0, &n, &n, &n));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layouts_python_assumes(tmp_path):
    src = tmp_path / "abi_originals.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_originals")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    i, o, t, d = OR.hc_sr_originals_input, OR.hc_sr_originals_output, OR.hc_sr_originals_text_counts, OR.ORIGINAL_DTYPE
    assert out["sizes"] == f"{d.itemsize} {C.sizeof(i)} {C.sizeof(o)} {C.sizeof(t)}"
    assert d.itemsize == 24 and C.sizeof(i) == 17 * 8 and C.sizeof(o) == 48 and C.sizeof(t) == 24
    assert out["entry"] == " ".join(str(d.fields[k][1]) for k in ("id", "index1", "index2", "len1", "len2", "paired", "forward"))
    assert out["offsets"] == (f"{i.n_cliques.offset} {i.n_srs.offset} {i.n_vertices.offset} {i.new_read_count.offset} {i.first_it.offset} "
                              f"{o.n_entries.offset} {o.ms_copy.offset}")
    assert out["status"] == f"{OR.ORIG_OK} {OR.ORIG_EMPTY_SOURCE} {OR.ORIG_SEQ0_OF_PAIRED} {OR.ORIG_RANGE} {OR.SOME_FAILED}"
    assert out["rc"] == " ".join(["-1"] * 9)  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    inp, out, cn = OR.hc_sr_originals_input(), OR.hc_sr_originals_output(), OR.hc_sr_originals_text_counts()
    n = C.c_uint64()
    assert N.lib.hc_sr_originals_init(None) == -1
    assert N.lib.hc_sr_originals_load(None, None, None, 0) == -1
    assert N.lib.hc_sr_originals_fetch(None, None, 0, None, 0, C.byref(n), C.byref(n)) == -1
    assert N.lib.hc_sr_originals_next(None, C.byref(inp), C.byref(out)) == -1
    assert N.lib.hc_sr_originals_write_text(None, C.byref(cn)) == -1
    assert N.lib.hc_sr_originals_text_fetch(None, 0, 0, None) == -1
    assert N.lib.hc_host_sr_originals_next(None, None, 0, C.byref(inp), C.byref(out), None, 0, 1) == -1
    assert N.lib.hc_host_sr_originals_text(None, None, 0, None, 0, C.byref(n)) == -1
    assert N.lib.hc_host_sr_originals_parse(None, 5, None, 0, None, 0, C.byref(n), C.byref(n), C.byref(n)) == -1
    # an input of nothing with nowhere to put the offsets is refused too
    off = (C.c_uint64 * 1)(0)
    assert N.lib.hc_host_sr_originals_next(off, None, 0, C.byref(inp), C.byref(out), None, 0, 1) == -1


def test_comments_cite_the_reference_and_state_the_order_contract():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int \w+\([^;]*;\s*)?int " + name + r"\(", src, re.S)
        assert m, name + ": no comment in front of the declaration"
    section = src[src.index("the original-read index maps on the device, and subreads.txt"):]
    for cite in (":750-806", ":938-949", ":1161-1216", ":1312-1369", ":1449-1463", ":1489-1503", ":1537-1551", "OverlapGraph.cpp:768-846", ":807-838",
                 "Read.h:145-149", ":1178", "ASCENDING ORIGINAL ID", "unordered_map", "never set nor printed", "Left to the caller", "HC_ERR_STATE",
                 "HC_SR_ORIG_SOME_FAILED", "stable radix sort", "count, then fetch"):
        assert cite in section, cite
    # the maps are no longer listed as the caller's by the calls in front of this one
    before = src[:src.index("the original-read index maps on the device, and subreads.txt")]
    assert not re.search(r"Left to the caller:[^.]*original-index maps", before)
    assert before.count("hc_sr_originals_next") >= 5
