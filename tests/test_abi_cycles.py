"""hc_graph_sort_edges, hc_graph_remove_cycles, hc_graph_fetch_cycle_pairs (include/hcedge.h) and the host mirror
(include/hcedge_host.h) as C99: the headers compile in a plain C program that fills the structures and calls them, the layout is the
one the Python structures assume, the symbols are exported, the comment states the reference's rules, and the calls answer NULL
arguments with HC_ERR_ARG (no GPU is touched; the refusals that need a context are checked in tests/test_gpu_cycles.py)."""
import ctypes as C
import os
import re
import subprocess

from haploconduct_amd import _native as N
from haploconduct_amd import cycles as CY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hc_graph_sort_edges", "hc_graph_remove_cycles", "hc_graph_fetch_cycle_pairs", "hc_host_graph_remove_cycles", "hc_host_graph_find_cycles",
         "hc_host_cycles_perm_table")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "hcedge_host.h"
int main(void) {
    hc_cycles_settings st = {1, 0};
    hc_cycles_counts cn;
    hc_sort_counts sc;
    uint64_t n = 0;
    printf("sizes %lu %lu %lu\n", (unsigned long)sizeof st, (unsigned long)sizeof cn, (unsigned long)sizeof sc);
    printf("offsets %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(hc_cycles_counts, backedge_count), (unsigned long)offsetof(hc_cycles_counts, try_size),
           (unsigned long)offsetof(hc_cycles_counts, n_flagged_components), (unsigned long)offsetof(hc_cycles_counts, status),
           (unsigned long)offsetof(hc_cycles_counts, bad_pos), (unsigned long)offsetof(hc_cycles_counts, ms_first_device));
    printf("status %u %u %u %u\n", HC_CYCLES_OK, HC_CYCLES_NAN_KEY, HC_CYCLES_NOT_SORTED, HC_CYCLES_TRIES);
    printf("rc %d %d %d %d %d\n", hc_graph_sort_edges(NULL, NULL, 0, &sc), hc_graph_remove_cycles(NULL, &st, &cn), hc_graph_fetch_cycle_pairs(NULL, NULL, 0, &n),
           hc_host_graph_remove_cycles(NULL, NULL, NULL, NULL, 0, &st, 1, NULL, NULL, NULL, NULL, NULL, NULL, 0, &cn),
           hc_host_graph_find_cycles(NULL, NULL, NULL, 0, 21, NULL, 0, &n));
    return 0;
}
'''


def test_calls_compile_as_c99_with_the_layout_python_assumes(tmp_path):
    src = tmp_path / "abi_cycles.c"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "abi_cycles")
    libdir = os.path.dirname(N.lib._name)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L", libdir, "-lhcedge", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    out = dict(l.split(" ", 1) for l in r.stdout.strip().split("\n"))
    s, t, q = CY.hc_cycles_settings, CY.hc_cycles_counts, CY.hc_sort_counts
    assert out["sizes"] == f"{C.sizeof(s)} {C.sizeof(t)} {C.sizeof(q)}" == "8 280 16"
    assert out["offsets"] == (f"{t.backedge_count.offset} {t.try_size.offset} {t.n_flagged_components.offset} {t.status.offset} {t.bad_pos.offset} "
                              f"{t.ms_first_device.offset}") == "16 40 200 224 232 240"
    assert out["status"] == "0 1 2 20" and CY.CYCLES_STATUS == ("OK", "NAN_KEY", "NOT_SORTED") and CY.TRIES == 20
    assert out["rc"] == "-1 -1 -1 -1 -1"  # HC_ERR_ARG


def test_symbols_are_exported_and_refuse_null_arguments_from_python():
    for name in NAMES:
        assert hasattr(N.lib, name), name
    st, cn, sc, n = CY.hc_cycles_settings(1, 0), CY.hc_cycles_counts(), CY.hc_sort_counts(), C.c_uint64()
    assert N.lib.hc_graph_sort_edges(None, None, 0, C.byref(sc)) == -1
    assert N.lib.hc_graph_remove_cycles(None, C.byref(st), C.byref(cn)) == -1
    assert N.lib.hc_graph_fetch_cycle_pairs(None, None, 0, C.byref(n)) == -1
    assert N.lib.hc_host_cycles_perm_table(3, None) == -1 and N.lib.hc_host_cycles_perm_table(0, None) == 0


def test_comment_states_the_reference_rules():
    src = open(os.path.join(ROOT, "include", "hcedge.h")).read()
    host = open(os.path.join(ROOT, "include", "hcedge_host.h")).read()
    for name in NAMES[:3]:
        assert re.search(r"int " + name + r"\(", src), name
    for name in NAMES[3:]:
        assert re.search(r"int " + name + r"\(", host), name
    section = src[src.index("the second sortEdges and cycleRemovalHeuristic on the device graph"):src.index("graph.txt, digraph.txt and the GFA files")]
    for cite in ("src/OverlapGraph.cpp:722-764", "src/GraphAlgos.cpp:150-176, 352-541", "src/OverlapGraph.cpp:548-562", ":104-147", "src/ViralQuasispecies.cpp:360-366",
                 "(in-degree, id)", "pos1 ascending", "score descending", "len0 descending", "mismatch_rate ascending", "std::random_shuffle", "never reseeded",
                 "self-loop", "20 otherwise", "strictly smallest", "FIRST record", "first u of adj_in[v]", "branching_edges", "keeps its later records",
                 "no file when there is none", "graph_depth", "at most 16 records", "HC_CYCLES_NOT_SORTED", "HC_CYCLES_NAN_KEY", "tied lists"):
        assert cite in section, cite
