"""include/hcsr.h as C99: the header compiles in a plain C program, the record layouts are what the Python views say, and a call
through it (the host mirror and the edge-merge helper; no GPU) gives the consensus of a two-read merge."""
import ctypes as C
import os
import subprocess

import numpy as np

from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "hcsr.h"
int main(void) {
    printf("member %zu %zu %zu %zu %zu\n", sizeof(hc_sr_member), offsetof(hc_sr_member, read), offsetof(hc_sr_member, pos), offsetof(hc_sr_member, seq),
           offsetof(hc_sr_member, rev));
    printf("layout %zu %zu %zu %zu\n", sizeof(hc_sr_layout), offsetof(hc_sr_layout, first_member), offsetof(hc_sr_layout, n_members),
           offsetof(hc_sr_layout, total_len));
    printf("settings %zu %zu %zu %zu %zu %zu\n", sizeof(hc_sr_settings), offsetof(hc_sr_settings, min_qual), offsetof(hc_sr_settings, min_clique_size),
           offsetof(hc_sr_settings, error_correction), offsetof(hc_sr_settings, subreads_needed), offsetof(hc_sr_settings, n_threads));
    printf("stats %zu %zu %zu %zu\n", sizeof(hc_sr_stats), offsetof(hc_sr_stats, n_host_columns), offsetof(hc_sr_stats, ms_device),
           offsetof(hc_sr_stats, ms_host_finish));
    /* two single-end reads, the second 4 bases into the first */
    const uint8_t bases[] = "ACGTACGTACGTACGTTT", quals[] = "IIIIIIIIII55555555";
    const uint64_t seq_off[3] = {0, 10, 18};
    const uint32_t first[3] = {0, 1, 2}, lens[2] = {10, 8};
    hc_edge_rec e;
    memset(&e, 0, sizeof e);
    e.read1 = 0; e.read2 = 1; e.v1 = 0; e.v2 = 1; e.ori1 = 1; e.ori2 = 1; e.pos1 = 4;
    hc_sr_layout lay; hc_sr_member mem[2]; uint64_t bad = 0;
    if (hc_host_sr_edge_layouts(&e, 1, lens, NULL, 2, &lay, mem, &bad) != HC_OK) return 2;
    hc_sr_settings st = {0.5, 2, 0, 0, 1};
    int32_t ret; uint32_t status; uint64_t off[2], nb = 0; uint8_t seq[32], qual[32]; hc_sr_stats stats;
    int rc = hc_host_sr_consensus(bases, quals, seq_off, first, 2, &lay, 1, mem, 2, &st, &ret, &status, off, NULL, NULL, 0, &nb, NULL);
    if (rc == HC_OK || nb != 12) return 3; /* count first ... */
    rc = hc_host_sr_consensus(bases, quals, seq_off, first, 2, &lay, 1, mem, 2, &st, &ret, &status, off, seq, qual, sizeof seq, &nb, &stats);
    if (rc != HC_OK || status != HC_SR_OK || ret != 0) return 4; /* ... then fetch */
    printf("cons %.*s %.*s %d\n", (int)nb, (const char*)seq, (int)nb, (const char*)qual, (int)stats.n_columns);
    uint8_t col[2];
    if (hc_host_sr_column((const uint8_t*)"TA", (const uint8_t*)"55", 2, 0.3, col) != 1 || col[0] != 'A') return 5;
    hc_sr_member wrong = mem[1]; wrong.read = 7; mem[1] = wrong;
    rc = hc_host_sr_consensus(bases, quals, seq_off, first, 2, &lay, 1, mem, 2, &st, &ret, &status, off, seq, qual, sizeof seq, &nb, NULL);
    if (rc != HC_OK || status != HC_SR_BAD_LAYOUT || nb != 0) return 6;
    return 0;
}
'''


def test_hcsr_header_is_c99_and_calls_through(tmp_path):
    src = tmp_path / "abi_sr.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_sr")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    m, l = SR.SR_MEMBER_DTYPE, SR.SR_LAYOUT_DTYPE
    assert out["member"] == f"{m.itemsize} {m.fields['read'][1]} {m.fields['pos'][1]} {m.fields['seq'][1]} {m.fields['rev'][1]}"
    assert out["layout"] == f"{l.itemsize} {l.fields['first_member'][1]} {l.fields['n_members'][1]} {l.fields['total_len'][1]}"
    s = N.hc_sr_settings
    assert out["settings"] == f"{C.sizeof(s)} {s.min_qual.offset} {s.min_clique_size.offset} {s.error_correction.offset} {s.subreads_needed.offset} {s.n_threads.offset}"
    t = N.hc_sr_stats
    assert out["stats"] == f"{C.sizeof(t)} {t.n_host_columns.offset} {t.ms_device.offset} {t.ms_host_finish.offset}"
    seq, qual, n = out["cons"].split(" ")
    assert seq == "ACGTACGTACTT" and len(qual) == 12 and n == "12"


def test_every_entry_point_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    assert src.count("SRBuilder.cpp:") >= 3 and src.count(":") > 30
    for name in ("hc_sr_consensus", "hc_host_sr_consensus", "hc_host_sr_column", "hc_host_sr_table", "hc_host_sr_edge_layouts"):
        assert name in src and hasattr(N.lib, name)


def test_device_call_without_reads_or_arguments_is_an_error():
    n = C.c_uint64()
    assert N.lib.hc_sr_consensus(None, None, 0, None, 0, None, None, None, None, None, None, 0, C.byref(n), None) != 0
