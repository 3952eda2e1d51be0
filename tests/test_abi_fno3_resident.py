"""hc_fno3_from_originals, its two fetches and the host mirror in include/hcsr.h as C99: the header compiles in a plain C program that
fills the structures and calls the four, the layouts are the ones the Python structures and the numpy dtype assume (a 16-byte
candidate), the symbols are exported, the comment states the rule, and the calls answer NULL arguments with an error (no GPU is touched)."""
import ctypes as C
import os
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import originals as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_fno3_from_originals", "hc_fno3_text_fetch", "hc_fno3_candidates_fetch", "hc_host_fno3_from_originals")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
int main(void) {
    hc_fno3_resident_input in = {1, 2, 3, NULL, 6, 0, HC_FNO_NO_INCLUSIONS, 0};
    hc_fno3_resident_counts cn;
    hc_fno3_candidate cd = {0, 1, 7, HC_FNO3_CAND_AMBIGUOUS | HC_FNO3_CAND_LINE};
    uint64_t n = 0;
    printf("sizes %lu %lu %lu\n", (unsigned long)sizeof in, (unsigned long)sizeof cn, (unsigned long)sizeof cd);
    printf("input %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_fno3_resident_input, n_single), (unsigned long)offsetof(hc_fno3_resident_input, n_trivial),
           (unsigned long)offsetof(hc_fno3_resident_input, n_paired), (unsigned long)offsetof(hc_fno3_resident_input, walk_rank),
           (unsigned long)offsetof(hc_fno3_resident_input, original_readcount), (unsigned long)offsetof(hc_fno3_resident_input, max_combos),
           (unsigned long)offsetof(hc_fno3_resident_input, flags));
    printf("counts %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_fno3_resident_counts, n_lines), (unsigned long)offsetof(hc_fno3_resident_counts, n_bytes),
           (unsigned long)offsetof(hc_fno3_resident_counts, candidates), (unsigned long)offsetof(hc_fno3_resident_counts, n_combos),
           (unsigned long)offsetof(hc_fno3_resident_counts, n_ambiguous), (unsigned long)offsetof(hc_fno3_resident_counts, n_originals),
           (unsigned long)offsetof(hc_fno3_resident_counts, ms_device));
    printf("candidate %lu %lu %lu %lu %u\n", (unsigned long)offsetof(hc_fno3_candidate, a), (unsigned long)offsetof(hc_fno3_candidate, b),
           (unsigned long)offsetof(hc_fno3_candidate, original_id), (unsigned long)offsetof(hc_fno3_candidate, flags), cd.flags);
    printf("rc %d %d %d %d\n", hc_fno3_from_originals(NULL, &in, &cn), hc_fno3_text_fetch(NULL, 0, 0, NULL), hc_fno3_candidates_fetch(NULL, 0, 0, &cd),
           hc_host_fno3_from_originals(NULL, NULL, 0, NULL, &in, &cn, NULL, 0, &n, NULL, 0));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layouts_python_assumes(tmp_path):
    src = tmp_path / "abi_fno3_resident.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_fno3_resident")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    i, c, d = OR.hc_fno3_resident_input, OR.hc_fno3_resident_counts, OR.FNO3_CANDIDATE_DTYPE
    assert out["sizes"] == f"{C.sizeof(i)} {C.sizeof(c)} {d.itemsize}"
    assert C.sizeof(i) == 56 and C.sizeof(c) == 56 and d.itemsize == 16
    assert out["input"] == " ".join(str(getattr(i, k).offset) for k in ("n_single", "n_trivial", "n_paired", "walk_rank", "original_readcount", "max_combos", "flags"))
    assert out["counts"] == " ".join(str(getattr(c, k).offset) for k in ("n_lines", "n_bytes", "candidates", "n_combos", "n_ambiguous", "n_originals", "ms_device"))
    assert out["candidate"] == " ".join(str(d.fields[k][1]) for k in ("a", "b", "original_id", "flags")) + f" {OR.CAND_AMBIGUOUS | OR.CAND_LINE}"
    assert out["rc"] == " ".join(["-1"] * 4)  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    inp, cn, n = OR.hc_fno3_resident_input(), OR.hc_fno3_resident_counts(), C.c_uint64()
    assert N.lib.hc_fno3_from_originals(None, C.byref(inp), C.byref(cn)) == -1
    assert N.lib.hc_fno3_text_fetch(None, 0, 0, None) == -1
    assert N.lib.hc_fno3_candidates_fetch(None, 0, 0, None) == -1
    assert N.lib.hc_host_fno3_from_originals(None, None, 0, None, C.byref(inp), C.byref(cn), None, 0, C.byref(n), None, 0) == -1


def test_the_comment_states_the_rule_and_nothing_is_left_to_the_caller():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    assert "Left to the caller: FNO=3" not in src
    section = src[src.index("FNO=3 from the kept dict"):]
    for cite in ("FindNextOverlaps3.cpp:20-173", ":176-406", ":29-76", ":240-281", ":157-165", ":391", "SRBuilder.cpp:1142-1233", "SMALLEST ID", "AMBIGUOUS",
                 "WALK RANK", "d_l", "d_r", "ascending (walk rank of SR1, walk rank of SR2)", "stable radix sort", "HC_ERR_STATE", "HC_ERR_NOT_ON_DEVICE",
                 "HC_ERR_FORMAT", "original_readcount", "count, then fetch", "no atomics on the outputs"):
        assert cite in section, cite
    for name in NAMES:
        assert ("int " + name + "(") in section, name
