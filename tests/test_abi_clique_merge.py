"""The C ABI of the clique merge (include/hcsr.h) without a GPU: the header compiles as plain C99, the structure sizes and enum values are
the ones the Python views assume, the symbols are exported and refuse null arguments."""
import ctypes as C
import os
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import consensus as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdio.h>
#include <stddef.h>
#include "hcsr.h"
int main(void) {
    printf("stats %zu %zu %zu %zu %zu\n", sizeof(hc_sr_clique_stats), offsetof(hc_sr_clique_stats, n_filtered_layouts),
           offsetof(hc_sr_clique_stats, n_host_filters), offsetof(hc_sr_clique_stats, ms_layout), offsetof(hc_sr_clique_stats, ms_host_filter));
    printf("status %d %d %d\n", HC_SR_EDGE_BAD_GEOMETRY, HC_SR_CLIQUE_TOO_SMALL, HC_SR_CLIQUE_REPEATED_VERTEX);
    printf("filter %d %d %d %d\n", HC_SR_FILTER_NONE, HC_SR_FILTER_GROUPS, HC_SR_FILTER_STABLE, HC_SR_FILTER_HOST);
    printf("sub %zu\n", sizeof(hc_sr_subread_info));
    {
        uint32_t vertex[3] = {4, 5, 6}, filter = 9;
        int32_t endpos[3] = {10, 30, 20};
        uint8_t used[3] = {7, 7, 7};
        if (hc_host_sr_clique_filter(vertex, endpos, 3, 2, 4, 0, used, &filter) != HC_OK) return 2;
        printf("used %d %d %d %u\n", used[0], used[1], used[2], filter);
    }
    return 0;
}
'''


def test_header_is_plain_c_and_the_layouts_match(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "abi"
    lib_dir = os.path.join(ROOT, "haploconduct_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", lib_dir, "-lhcedge",
                    "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    S = N.hc_sr_clique_stats
    assert out[0] == f"stats {C.sizeof(S)} {S.n_filtered_layouts.offset} {S.n_host_filters.offset} {S.ms_layout.offset} {S.ms_host_filter.offset}"
    assert C.sizeof(S) == 64 and S.n_filtered_layouts.offset == C.sizeof(N.hc_sr_stats) == 32
    assert out[1] == f"status {SR.SR_EDGE_BAD_GEOMETRY} {SR.SR_CLIQUE_TOO_SMALL} {SR.SR_CLIQUE_REPEATED_VERTEX}" == "status 5 6 7"
    assert out[2] == f"filter {SR.SR_FILTER_NONE} {SR.SR_FILTER_GROUPS} {SR.SR_FILTER_STABLE} {SR.SR_FILTER_HOST}" == "filter 0 1 2 3"
    assert out[3] == f"sub {SR.SR_SUBREAD_DTYPE.itemsize}"
    assert out[4] == f"used 1 1 0 {SR.SR_FILTER_GROUPS}"  # num = 2: the base (the first entry too) and the largest endpos


def test_symbols_are_exported_and_refuse_null_arguments():
    for name in ("hc_sr_clique_merge", "hc_host_sr_clique_merge_layouts", "hc_host_sr_clique_filter", "hc_sr_clique_filter_on_host"):
        assert hasattr(N.lib, name), name
    assert N.lib.hc_sr_clique_filter_on_host(None, 1) == -1
    n = C.c_uint64(0)
    assert N.lib.hc_sr_clique_merge(None, None, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                    None, 0, C.byref(n), None) == -1
    assert N.lib.hc_host_sr_clique_merge_layouts(None, None, 0, None, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None,
                                                 None, None, None, None) == -1
    assert N.lib.hc_host_sr_clique_filter(None, None, 0, 0, 0, 0, None, None) == -1
