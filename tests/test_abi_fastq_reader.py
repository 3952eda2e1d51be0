"""hc_set_reads_from_fastq_text, hc_fastq_fetch and hc_fastq_set_chunk_bytes in include/hcedge.h as C99: the header compiles in a plain C
program that fills the structures and calls the three calls, the layouts are the ones the Python structures assume, the symbols are
exported, NULL arguments are answered with HC_ERR_ARG (no GPU is touched; hc_fastq_fetch's HC_ERR_STATE needs a context and is checked in
tests/test_gpu_fastq_reader.py), and the section's comment cites the reference lines and states the contracts."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import fastq_reader as FR
from haploconduct_amd import host  # noqa: F401  (binds hc_ec_fastq_on_device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_set_reads_from_fastq_text", "hc_fastq_fetch", "hc_fastq_set_chunk_bytes")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcedge.h"
#include "hcedge_host.h"
int main(void) {
    hc_fastq_text tx = {0};
    hc_fastq_counts cn;
    uint64_t ids[1], off[1];
    uint32_t first[1];
    tx.singles = "@1\nA\n+\nI\n";
    tx.n_singles = 10;
    tx.max_reads = 100000000;
    printf("sizes %lu %lu\n", (unsigned long)sizeof tx, (unsigned long)sizeof cn);
    printf("text %lu %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_fastq_text, singles), (unsigned long)offsetof(hc_fastq_text, n_singles),
           (unsigned long)offsetof(hc_fastq_text, paired1), (unsigned long)offsetof(hc_fastq_text, n_paired1), (unsigned long)offsetof(hc_fastq_text, paired2),
           (unsigned long)offsetof(hc_fastq_text, n_paired2), (unsigned long)offsetof(hc_fastq_text, ids_path), (unsigned long)offsetof(hc_fastq_text, max_reads));
    printf("counts %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_fastq_counts, n_reads), (unsigned long)offsetof(hc_fastq_counts, n_seq),
           (unsigned long)offsetof(hc_fastq_counts, n_single), (unsigned long)offsetof(hc_fastq_counts, n_paired), (unsigned long)offsetof(hc_fastq_counts, n_bytes),
           (unsigned long)offsetof(hc_fastq_counts, n_host_ids), (unsigned long)offsetof(hc_fastq_counts, err_record), (unsigned long)offsetof(hc_fastq_counts, err_file),
           (unsigned long)offsetof(hc_fastq_counts, ms_copy), (unsigned long)offsetof(hc_fastq_counts, ms_device), (unsigned long)offsetof(hc_fastq_counts, ms_plan));
    printf("rc %d %d %d %d %d\n", hc_set_reads_from_fastq_text(NULL, &tx, &cn), hc_set_reads_from_fastq_text(NULL, NULL, NULL),
           hc_fastq_fetch(NULL, ids, 1, off, first, 0), hc_fastq_set_chunk_bytes(NULL, 4096), hc_ec_fastq_on_device(0));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layouts_python_assumes(tmp_path):
    src = tmp_path / "abi_fastq_reader.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_fastq_reader")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    t, c = FR.hc_fastq_text, FR.hc_fastq_counts
    assert out["sizes"] == f"{C.sizeof(t)} {C.sizeof(c)}" == "64 72"
    assert out["text"] == " ".join(str(getattr(t, k).offset) for k, _ in t._fields_) == "0 8 16 24 32 40 48 56"
    names = [k for k, _ in c._fields_ if k != "reserved"]
    assert out["counts"] == " ".join(str(getattr(c, k).offset) for k in names) == "0 4 8 12 16 24 32 40 48 56 64"
    assert out["rc"] == "-1 -1 -1 -1 0"  # HC_ERR_ARG; the stage's switch needs no device


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES + ("hc_ec_fastq_on_device", "hc_ec_fastq_was_on_device", "hc_ec_get_read_seq"):
        assert hasattr(N.lib, name), name
    tx, cn = FR.hc_fastq_text(), FR.hc_fastq_counts()
    assert N.lib.hc_set_reads_from_fastq_text(None, C.byref(tx), C.byref(cn)) == -1
    assert N.lib.hc_fastq_fetch(None, None, 0, None, None, 0) == -1
    assert N.lib.hc_fastq_set_chunk_bytes(None, 0) == -1
    assert b"null" in N.lib.hc_last_error()
    assert N.lib.hc_ec_get_read_seq(None, 0, 0, 0, None, 0, None) == -1 and N.lib.hc_ec_fastq_was_on_device(None) == 0


def test_comments_cite_the_reference_and_state_the_contracts():
    src = open(os.path.join(ROOT, "include", "hcedge.h")).read()
    for name in NAMES:
        assert re.search(r"int " + name + r"\(", src), name
    start = src.index("the FASTQ files' text read on the device into the read store")
    assert start > src.index("int hc_set_reads(")  # beside hc_set_reads
    section = src[start:src.index("int hc_fastq_set_chunk_bytes(")]
    for cite in ("src/FastqStorage.cpp:41-57, 92-152, 154-235", "src/FastqStorage.h:58-98", "src/Types.h:99-102", "count, then fetch", "IN THIS ORDER",
                 "(1)", "(2)", "(3)", "(4)", "(5)", "HC_ERR_NOT_ON_DEVICE", "device_mask", "2^32 - 4096", "HC_ERR_STATE", "HC_ERR_ARG", "n_host_ids",
                 "[1-9][0-9]{0,17}", "hc_sr_keep_device", "the old store stays usable", "2^28"):
        assert cite in section, cite
    hostsrc = open(os.path.join(ROOT, "include", "hcedge_host.h")).read()
    assert re.search(r"/\*((?:(?!\*/).)*)\*/\s*int hc_ec_fastq_on_device\(", hostsrc, re.S)
    assert "not an environment knob" in hostsrc
