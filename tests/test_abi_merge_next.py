"""hc_sr_merge_next and hc_host_sr_merge_next in include/hcsr.h as C99: the header compiles in a plain C program that names the two calls and
fills the three structures, the layouts are the ones the Python structures assume, the symbols are exported, the comments cite the reference
and say what stays with the caller, and the device call answers a NULL context with an error (no GPU is touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import merge_next as MN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_sr_merge_next", "hc_host_sr_merge_next")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
typedef int (*dev_fn)(hc_ctx*, const hc_sr_merge_next_input*, const hc_sr_merge_next_settings*, hc_sr_merge_next_output*);
typedef int (*host_fn)(const hc_settings*, const uint8_t*, const uint8_t*, const uint64_t*, const uint32_t*, uint32_t, const uint8_t*, const uint8_t*, uint64_t,
                       const hc_sr_merge_next_input*, const hc_sr_merge_next_settings*, hc_sr_merge_next_output*, uint8_t*, uint8_t*, uint64_t, uint64_t*,
                       uint64_t*, uint32_t*);
int main(void) {
    dev_fn d = hc_sr_merge_next; /* the declared types are the documented ones */
    host_fn h = hc_host_sr_merge_next;
    hc_sr_merge_next_input in;
    hc_sr_merge_next_settings st = {0, 0, 0, 0, {0.99, 0.99, 15, 1}};
    hc_sr_merge_next_output out;
    printf("sizes %lu %lu %lu\n", (unsigned long)sizeof in, (unsigned long)sizeof st, (unsigned long)sizeof out);
    printf("offsets %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_sr_merge_next_input, n_members), (unsigned long)offsetof(hc_sr_merge_next_input, tip_reads),
           (unsigned long)offsetof(hc_sr_merge_next_settings, self), (unsigned long)offsetof(hc_sr_merge_next_output, n_srs),
           (unsigned long)offsetof(hc_sr_merge_next_output, counts), (unsigned long)offsetof(hc_sr_merge_next_output, ms_copy));
    printf("enums %d %d %d %d\n", HC_SR_MN_NONE, HC_SR_MN_PAIRED, HC_SR_MN_V_MERGED, HC_SR_MN_V_BAD);
    printf("rc %d %d\n", d(NULL, &in, &st, &out), h == NULL);
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layouts_python_assumes(tmp_path):
    src = tmp_path / "abi_merge_next.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_merge_next")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    i, s, o = MN.hc_sr_merge_next_input, MN.hc_sr_merge_next_settings, MN.hc_sr_merge_next_output
    assert out["sizes"] == f"{C.sizeof(i)} {C.sizeof(s)} {C.sizeof(o)}"
    assert C.sizeof(s) == 40
    assert out["offsets"] == f"{i.n_members.offset} {i.tip_reads.offset} {s.self.offset} {o.n_srs.offset} {o.counts.offset} {o.ms_copy.offset}"
    assert out["enums"] == f"{MN.MN_NONE} {MN.MN_PAIRED} {MN.MN_V_MERGED} {MN.MN_V_BAD}" == "0 5 0 6"
    rc, null = out["rc"].split()
    assert int(rc) == -1 and null == "0"  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    inp, st, out = MN.hc_sr_merge_next_input(), MN.hc_sr_merge_next_settings(), MN.hc_sr_merge_next_output()
    assert N.lib.hc_sr_merge_next(None, C.byref(inp), C.byref(st), C.byref(out)) == -1
    assert N.lib.hc_sr_merge_next(None, None, None, None) == -1
    nb = C.c_uint64()
    assert N.lib.hc_host_sr_merge_next(None, None, None, None, None, 0, None, None, 0, C.byref(inp), C.byref(st), C.byref(out), None, None, 0, C.byref(nb), None,
                                       None) == -1


def test_comments_cite_the_reference_and_say_what_stays_with_the_caller():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", src, re.S)
        assert m, name + ": no comment in front of the declaration"
    section = src[src.index("the rest of mergeAlongEdges in one call"):]
    for cite in (":981-1001", ":1260-1277", ":1282-1373", ":911-935", ":872-955", "N_THREADS = 1", "Left to the caller", "subreads.txt",
                 "removed_tip_sequences.fastq", "cliques of more than two vertices", "HC_ERR_STATE", "HC_SR_NEXT_EMPTY"):
        assert cite in section, cite
    # every field of the three structures carries a comment with a line of the reference or the call it comes from
    for struct in ("hc_sr_merge_next_input", "hc_sr_merge_next_settings"):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct, src, re.S).group(1)
        for line in body.split("\n"):
            if ";" in line and "/*" in line:
                assert re.search(r":\d+|hc_sr_edge_merge|entries of", line), line
    # the pieces are no longer listed as the caller's
    assert "the trivial-entry list of :1260-1373. */" not in src
