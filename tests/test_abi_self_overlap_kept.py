"""The kept-bytes form of the self-overlap merge in include/hcsr.h (hc_sr_merge_self_overlaps_kept, hc_sr_kept_load, hc_sr_kept_fetch) as
C99: the header compiles in a plain C program that names the three calls, the symbols are exported, their comments cite the reference and
say what stays with the caller, and each call answers a NULL context with an error (no GPU is touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_sr_merge_self_overlaps_kept", "hc_sr_kept_load", "hc_sr_kept_fetch")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
typedef int (*kept_fn)(hc_ctx*, const hc_sr_pair*, uint64_t, const hc_sr_self_settings*, int32_t*, double*, uint32_t*, uint64_t*, uint64_t*,
                       hc_sr_self_stats*);
typedef int (*load_fn)(hc_ctx*, const uint8_t*, const uint8_t*, uint64_t);
typedef int (*fetch_fn)(hc_ctx*, uint64_t, uint64_t, uint8_t*, uint8_t*, uint64_t*);
int main(void) {
    kept_fn k = hc_sr_merge_self_overlaps_kept; /* the declared types are the documented ones */
    load_fn l = hc_sr_kept_load;
    fetch_fn f = hc_sr_kept_fetch;
    hc_sr_self_settings st = {0.99, 0.99, 15, 1};
    uint64_t off[1] = {7}, n_out = 7, n_kept = 7;
    uint8_t b[4] = {0, 0, 0, 0};
    int rc[3];
    rc[0] = k(NULL, NULL, 0, &st, NULL, NULL, NULL, off, &n_out, NULL);
    rc[1] = l(NULL, b, b, 4);
    rc[2] = f(NULL, 0, 4, b, b, &n_kept);
    printf("rc %d %d %d ok %d\n", rc[0], rc[1], rc[2], HC_OK);
    return 0;
}
'''


def test_kept_calls_compile_as_c99_and_refuse_a_null_context(tmp_path):
    src = tmp_path / "abi_srself_kept.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_srself_kept")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    w = r.stdout.split()
    assert w[0] == "rc" and all(int(x) != int(w[5]) for x in w[1:4]), r.stdout


def test_symbols_are_exported_and_refuse_a_null_context_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    n = C.c_uint64(5)
    assert N.lib.hc_sr_merge_self_overlaps_kept(None, None, 0, None, None, None, None, None, C.byref(n), None) != 0
    assert N.lib.hc_sr_kept_load(None, None, None, 0) != 0
    assert N.lib.hc_sr_kept_fetch(None, 0, 0, None, None, C.byref(n)) != 0


def test_comments_cite_the_reference_and_say_what_stays_with_the_caller():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", src, re.S)
        assert m, name + ": no comment in front of the declaration"
        text = m.group(1)
        assert "src/SRBuilder.cpp" in text, name + ": no citation of the reference"
        assert "Left to the caller" in text, name + ": what stays with the caller is not said"
    kept = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int hc_sr_merge_self_overlaps_kept\(", src, re.S).group(1)
    assert ":911-949" in kept and "test_N_rate" in kept and "ABSOLUTE" in kept and "HC_ERR_STATE" in kept
    # the piece is no longer listed as missing
    assert "a device-input form of hc_sr_merge_self_overlaps" not in src
