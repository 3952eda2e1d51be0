"""hc_sr_clique_next, hc_host_sr_clique_next and hc_host_sr_clique_select in include/hcsr.h as C99: the header compiles in a plain C program
that names the three calls and fills the three structures, the layouts are the ones the Python structures assume, the symbols are exported,
the comments cite the reference and state the call's own tie order, and the calls answer NULL arguments with an error (no GPU is
touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import clique_next as CN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_sr_clique_next", "hc_host_sr_clique_next", "hc_host_sr_clique_select")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
typedef int (*dev_fn)(hc_ctx*, const hc_sr_clique_next_input*, const hc_sr_clique_next_settings*, hc_sr_clique_next_output*);
typedef int (*host_fn)(const hc_settings*, const uint8_t*, const uint8_t*, const uint64_t*, const uint32_t*, uint32_t, const uint8_t*, const uint8_t*, uint64_t,
                       const hc_sr_clique_next_input*, const hc_sr_clique_next_settings*, hc_sr_clique_next_output*, uint8_t*, uint8_t*, uint64_t, uint64_t*,
                       uint64_t*, uint32_t*);
typedef int (*select_fn)(const uint64_t*, const uint32_t*, uint64_t, uint64_t, uint32_t, int, uint64_t*, uint32_t*, uint64_t*, uint64_t*, uint64_t*);
int main(void) {
    dev_fn d = hc_sr_clique_next; /* the declared types are the documented ones */
    host_fn h = hc_host_sr_clique_next;
    select_fn s = hc_host_sr_clique_select;
    hc_sr_clique_next_input in;
    hc_sr_clique_next_settings st = {0, 0, {0.99, 0.99, 15, 1}};
    hc_sr_clique_next_output out;
    uint64_t n = 0;
    printf("sizes %lu %lu %lu\n", (unsigned long)sizeof in, (unsigned long)sizeof st, (unsigned long)sizeof out);
    printf("offsets %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_sr_clique_next_input, n_cliques),
           (unsigned long)offsetof(hc_sr_clique_next_input, n_members), (unsigned long)offsetof(hc_sr_clique_next_input, n_vertices),
           (unsigned long)offsetof(hc_sr_clique_next_settings, self), (unsigned long)offsetof(hc_sr_clique_next_output, n_srs),
           (unsigned long)offsetof(hc_sr_clique_next_output, counts), (unsigned long)offsetof(hc_sr_clique_next_output, ms_copy));
    printf("rc %d %d %d\n", d(NULL, &in, &st, &out), h == NULL, s(NULL, NULL, 0, 0, 2, 0, NULL, NULL, NULL, &n, &n));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layouts_python_assumes(tmp_path):
    src = tmp_path / "abi_clique_next.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_clique_next")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    i, s, o = CN.hc_sr_clique_next_input, CN.hc_sr_clique_next_settings, CN.hc_sr_clique_next_output
    assert out["sizes"] == f"{C.sizeof(i)} {C.sizeof(s)} {C.sizeof(o)}"
    assert C.sizeof(s) == 32 and C.sizeof(i) == 15 * 8
    assert out["offsets"] == (f"{i.n_cliques.offset} {i.n_members.offset} {i.n_vertices.offset} {s.self.offset} {o.n_srs.offset} {o.counts.offset} "
                              f"{o.ms_copy.offset}")
    assert out["rc"] == "-1 0 -1"  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    inp, st, out = CN.hc_sr_clique_next_input(), CN.hc_sr_clique_next_settings(), CN.hc_sr_clique_next_output()
    assert N.lib.hc_sr_clique_next(None, C.byref(inp), C.byref(st), C.byref(out)) == -1
    assert N.lib.hc_sr_clique_next(None, None, None, None) == -1
    nb = C.c_uint64()
    assert N.lib.hc_host_sr_clique_next(None, None, None, None, None, 0, None, None, 0, C.byref(inp), C.byref(st), C.byref(out), None, None, 0, C.byref(nb), None,
                                        None) == -1
    assert N.lib.hc_host_sr_clique_select(None, None, 0, 0, 2, 0, None, None, None, C.byref(nb), C.byref(nb)) == -1


def test_comments_cite_the_reference_and_state_the_tie_order():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", src, re.S)
        assert m, name + ": no comment in front of the declaration"
    section = src[src.index("the rest of cliquesToSuperreads in one call"):]
    for cite in (":981-1001", ":1122-1136", ":1145-1222", ":911-935", ":872-955", ":1056-1084", "N_THREADS = 1", "Left to the caller", "subreads.txt",
                 "DESCENDING position", "stable sort", "FindNextOverlaps.cpp:900-913", "HC_ERR_STATE", "HC_SR_NEXT_EMPTY", "hc_sr_merge_next"):
        assert cite in section, cite
    # the gap is no longer listed as the caller's
    assert "a clique form of\n * hc_sr_merge_next" not in src and "from ITS outputs are not built" not in src
