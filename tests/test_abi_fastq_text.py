"""The hc_sr_fastq_* calls and their host mirrors in include/hcsr.h as C99: the header compiles in a plain C program that calls the four calls
and fills the structure, the layout is the one the Python structure assumes, the symbols are exported, the section's comment cites the
reference and states the ascending-id argument, the append note and the count-then-fetch contract, and the calls answer NULL arguments with
HC_ERR_ARG (no GPU is touched)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import fastq_text as FQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_sr_fastq_write_text", "hc_sr_fastq_text_fetch", "hc_host_sr_fastq_text", "hc_host_sr_fastq_tips_text")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
int main(void) {
    hc_sr_fastq_counts cn;
    uint64_t n = 0;
    int files[4] = {HC_SR_FASTQ_SINGLES, HC_SR_FASTQ_PAIRED1, HC_SR_FASTQ_PAIRED2, HC_SR_FASTQ_TIPS};
    printf("sizes %lu\n", (unsigned long)sizeof cn);
    printf("offsets %lu %lu %lu\n", (unsigned long)offsetof(hc_sr_fastq_counts, n_records), (unsigned long)offsetof(hc_sr_fastq_counts, n_bytes),
           (unsigned long)offsetof(hc_sr_fastq_counts, ms_device));
    printf("files %d %d %d %d\n", files[0], files[1], files[2], files[3]);
    printf("rc %d %d %d %d\n", hc_sr_fastq_write_text(NULL, NULL, 0, NULL, 0, &cn), hc_sr_fastq_text_fetch(NULL, 0, 0, 0, NULL),
           hc_host_sr_fastq_text(NULL, NULL, NULL, NULL, 0, 0, NULL, 0, &n), hc_host_sr_fastq_tips_text(NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, 0, &n));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layout_python_assumes(tmp_path):
    src = tmp_path / "abi_fastq_text.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_fastq_text")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    t = FQ.hc_sr_fastq_counts
    assert out["sizes"] == str(C.sizeof(t)) == "72"
    assert out["offsets"] == f"{t.n_records.offset} {t.n_bytes.offset} {t.ms_device.offset}" == "0 32 64"
    assert out["files"] == f"{FQ.FASTQ_SINGLES} {FQ.FASTQ_PAIRED1} {FQ.FASTQ_PAIRED2} {FQ.FASTQ_TIPS}"
    assert out["rc"] == " ".join(["-1"] * 4)  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    cn, n = FQ.hc_sr_fastq_counts(), C.c_uint64()
    assert N.lib.hc_sr_fastq_write_text(None, None, 0, None, 0, C.byref(cn)) == -1
    assert N.lib.hc_sr_fastq_text_fetch(None, 0, 0, 0, None) == -1
    assert N.lib.hc_host_sr_fastq_text(None, None, None, None, 0, 0, None, 0, C.byref(n)) == -1
    assert N.lib.hc_host_sr_fastq_tips_text(None, None, None, None, 0, None, 0, None, 0, C.byref(n)) == -1
    # nowhere to put the count is refused too
    off, first = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(0)
    assert N.lib.hc_host_sr_fastq_text(None, None, off, first, 0, 0, None, 0, None) == -1
    assert N.lib.hc_host_sr_fastq_text(None, None, off, first, 0, 0, None, 0, C.byref(n)) == 0 and n.value == 0  # an empty store is no error


def test_comments_cite_the_reference_and_state_the_contracts():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in NAMES:
        assert re.search(r"int " + name + r"\(", src), name
    start = src.index("singles.fastq, paired1.fastq, paired2.fastq and removed_tip_sequences.fastq from the device")
    assert start > src.index("the original-read index maps on the device, and subreads.txt")  # behind the originals section
    section = src[start:]
    for cite in (":1386-1414", ":1434-1447", ":1484-1487", ":1528-1535", ":1302", ":1309", ":1142", ":1231-1233", ":1280", ":1377-1378",
                 "ascending id", "append mode", "appends or truncates", "count, then fetch", "FORWARD", "HC_ERR_STATE", "HC_ERR_ARG",
                 "Left to the caller", "64-bit"):
        assert cite in section, cite
    # the mirrors and the fetch carry comments of their own
    for name in ("hc_sr_fastq_text_fetch", "hc_host_sr_fastq_text", "hc_host_sr_fastq_tips_text"):
        assert re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", src, re.S), name + ": no comment in front of the declaration"
    # the older sections point to the new call instead of leaving the text to the caller
    before = src[:start]
    assert not re.search(r"Left to the caller: the FASTQ text", before)
    assert before.count("hc_sr_fastq_write_text") >= 5
