"""The self-overlap part of include/hcsr.h as C99: the header compiles in a plain C program, the record layouts are what the Python views
say (24 bytes for hc_sr_pair), and a call of the host mirror through it (no GPU) merges a pair."""
import ctypes as C
import os
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "hcsr.h"
int main(void) {
    printf("pair %zu %zu %zu %zu %zu\n", sizeof(hc_sr_pair), offsetof(hc_sr_pair, off1), offsetof(hc_sr_pair, off2), offsetof(hc_sr_pair, len1),
           offsetof(hc_sr_pair, len2));
    printf("settings %zu %zu %zu %zu %zu\n", sizeof(hc_sr_self_settings), offsetof(hc_sr_self_settings, min_score), offsetof(hc_sr_self_settings, min_qual),
           offsetof(hc_sr_self_settings, min_overlap), offsetof(hc_sr_self_settings, n_threads));
    printf("stats %zu %zu %zu %zu %zu %zu\n", sizeof(hc_sr_self_stats), offsetof(hc_sr_self_stats, n_merged), offsetof(hc_sr_self_stats, n_host_pairs),
           offsetof(hc_sr_self_stats, n_offsets), offsetof(hc_sr_self_stats, ms_device), offsetof(hc_sr_self_stats, ms_host));
    printf("enum %d %d %d %d\n", HC_SR_SELF_NONE, HC_SR_SELF_MERGED, HC_SR_SELF_BAD_PAIR, HC_SR_SELF_BAD_SYMBOL);
    /* mate 2 starts 6 bases into mate 1; a second pair that does not overlap; a third with an empty mate */
    const uint8_t seq[] = "ACGTACGTACGTACGTACGTAGGGTACGTACGTACGTAGGTTTCCCCCCCCCCCCCCCCCCCC";
    uint8_t qual[sizeof seq];
    memset(qual, 'I', sizeof qual);
    const hc_sr_pair pairs[3] = {{0, 23, 23, 20}, {0, 43, 23, 20}, {0, 23, 23, 0}};
    hc_settings ec;
    memset(&ec, 0, sizeof ec);
    hc_sr_self_settings st = {0.99, 0.99, 15, 1};
    int32_t pos[3]; double score[3]; uint32_t status[3]; uint64_t off[4], n_out = 0; uint8_t ms[64], mq[64]; hc_sr_self_stats stats;
    int rc = hc_host_sr_merge_self_overlaps(&ec, seq, qual, 63, pairs, 3, &st, pos, score, status, off, NULL, NULL, 0, &n_out, NULL);
    if (rc == HC_OK || n_out != 26) return 3; /* count first ... */
    rc = hc_host_sr_merge_self_overlaps(&ec, seq, qual, 63, pairs, 3, &st, pos, score, status, off, ms, mq, sizeof ms, &n_out, &stats);
    if (rc != HC_OK) return 4; /* ... then fetch */
    if (status[0] != HC_SR_SELF_MERGED || pos[0] != 6 || !(score[0] > 0.99) || off[1] != 26) return 5;
    if (status[1] != HC_SR_SELF_NONE || pos[1] != -1 || score[1] != 0 || status[2] != HC_SR_SELF_BAD_PAIR || off[3] != 26) return 6;
    if (stats.n_merged != 1 || stats.n_offsets != 16) return 7;
    printf("merged %.*s %.*s\n", (int)n_out, (const char*)ms, (int)n_out, (const char*)mq);
    return 0;
}
'''


def test_self_overlap_header_is_c99_and_calls_through(tmp_path):
    src = tmp_path / "abi_srself.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_srself")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    p = SR.SR_PAIR_DTYPE
    assert out["pair"] == f"24 {p.fields['off1'][1]} {p.fields['off2'][1]} {p.fields['len1'][1]} {p.fields['len2'][1]}" and p.itemsize == 24
    s = N.hc_sr_self_settings
    assert out["settings"] == f"{C.sizeof(s)} {s.min_score.offset} {s.min_qual.offset} {s.min_overlap.offset} {s.n_threads.offset}" and C.sizeof(s) == 24
    t = N.hc_sr_self_stats
    assert out["stats"] == f"{C.sizeof(t)} {t.n_merged.offset} {t.n_host_pairs.offset} {t.n_offsets.offset} {t.ms_device.offset} {t.ms_host.offset}"
    assert out["enum"] == f"{SR.SR_SELF_NONE} {SR.SR_SELF_MERGED} {SR.SR_SELF_BAD_PAIR} {SR.SR_SELF_BAD_SYMBOL}"
    seq, qual = out["merged"].split(" ")
    assert seq == "ACGTACGTACGTACGTACGTAGGTTT" and len(qual) == 26


def test_entry_points_cite_the_reference_and_say_what_stays_with_the_caller():
    src = open(os.path.join(ROOT, "include", "hcsr.h")).read()
    for name in ("hc_sr_merge_self_overlaps", "hc_host_sr_merge_self_overlaps"):
        assert name in src and hasattr(N.lib, name)
    assert "SRBuilder.cpp:872-955" in src and "EdgeCalculator.cpp:67-139" in src
    assert "test_N_rate" in src and ":911-949" in src and "tightening" in src


def test_device_call_without_arguments_is_an_error():
    n = C.c_uint64()
    assert N.lib.hc_sr_merge_self_overlaps(None, None, None, 0, None, 0, None, None, None, None, None, None, None, 0, C.byref(n), None) != 0
