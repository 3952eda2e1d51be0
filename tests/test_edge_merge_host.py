"""The host mirror of the edge merge (include/hcsr.h: hc_host_sr_edge_merge_layouts, hc_host_graph_merge_pairs) against the reference's
own sort_vertices / calcSubreadInfo / getEdgesForMerging (tests/golden/edge_merge.json, made by tests/golden/make_golden_edge_merge.py
with the genuine lines of constructSuperread's head), against hc_host_sr_edge_layouts on all-single-end input, and its refusals."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from haploconduct_amd import _native as N, consensus as SR, host
from tests import _edge_merge as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = EM.load_cases()


def mirror(case, pairs, ret=None, reads=None):
    edges, out_off, _, _ = EM.csr(case["V"], case["edges_in"])
    reads = reads or EM.random_reads(case["reads"], 3)
    return host.sr_edge_merge_layouts(edges, out_off, reads, pairs, case["vertex_read"], case["vertex_fwd"], ret)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_layouts_equal_the_reference(case):
    pairs, first, layouts, members = EM.golden_arrays(case)
    got = mirror(case, pairs)
    EM.assert_layouts(got, first, layouts, members, case["name"])
    # type, base and list order per pair, for a readable failure
    for i, p in enumerate(case["pairs"]):
        assert int(got.first_layout[i + 1] - got.first_layout[i]) == (2 if p["type"] == "p" else 1), p["pair"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_subread_infos_equal_the_reference(case):
    pairs, first, layouts, _ = EM.golden_arrays(case)
    n_variants = max(len(p["subreads"]) for p in case["pairs"])
    for k in range(n_variants):
        ret = np.zeros(layouts.size, np.int32)
        want = np.zeros((pairs.shape[0], 2), SR.SR_SUBREAD_DTYPE)
        for i, p in enumerate(case["pairs"]):
            t1, t2, a, b = p["subreads"][k % len(p["subreads"])]
            l0 = int(first[i])
            ret[l0] = t1
            if p["type"] == "p":
                ret[l0 + 1] = t2
            want[i, 0], want[i, 1] = tuple(a), tuple(b)
        got = mirror(case, pairs, ret)
        assert np.array_equal(got.subreads, want), (case["name"], k, np.flatnonzero((got.subreads != want).any(axis=1))[:5])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_merge_pairs_equal_the_reference(case):
    edges, out_off, _, _ = EM.csr(case["V"], case["edges_in"])
    got = host.graph_merge_pairs(edges, out_off)
    assert got.tolist() == case["merge_pairs"], case["name"]


def test_host_merge_pairs_counts_then_fetches():
    case = next(c for c in CASES if c["name"] == "chain")
    edges, out_off, _, _ = EM.csr(case["V"], case["edges_in"])
    import ctypes as C

    n = C.c_uint64(0)
    rc = N.lib.hc_host_graph_merge_pairs(edges.ctypes.data, out_off.ctypes.data, case["V"], None, 0, C.byref(n))
    assert rc != 0 and n.value == len(case["merge_pairs"])
    out = np.zeros((n.value, 2), np.uint32)
    assert N.lib.hc_host_graph_merge_pairs(edges.ctypes.data, out_off.ctypes.data, case["V"], out.ctypes.data, n.value, C.byref(n)) == 0
    assert out.tolist() == case["merge_pairs"]


def test_single_end_pairs_equal_hc_host_sr_edge_layouts():
    """Every all-single-end golden pair: the record getEdgeInfo finds, handed to hc_host_sr_edge_layouts, gives the same layout."""
    n = 0
    for case in CASES:
        edges, out_off, _, _ = EM.csr(case["V"], case["edges_in"])
        reads = EM.random_reads(case["reads"], 3)
        vr = case["vertex_read"]
        for p in case["pairs"]:
            a, b = sorted(p["pair"])
            if case["reads"][vr[a]][2] or case["reads"][vr[b]][2]:
                continue
            lst = edges[int(out_off[a]):int(out_off[a + 1])]
            rec = lst[lst["v2"] == b][:1]
            if rec.size == 0:
                lst = edges[int(out_off[b]):int(out_off[b + 1])]
                rec = lst[lst["v2"] == a][:1]
            if int(rec["read1"][0]) != vr[int(rec["v1"][0])]:
                continue  # hc_host_sr_edge_layouts takes the base from the vertices: only records whose read 1 is v1's read compare
            rec = rec.copy()
            rec["ori1"], rec["ori2"] = case["vertex_fwd"][int(rec["v1"][0])], case["vertex_fwd"][int(rec["v2"][0])]
            lay, mem = SR.edge_layouts(rec, reads)
            got = mirror(case, [p["pair"]], reads=reads)
            assert np.array_equal(got.layouts, lay) and np.array_equal(got.members, mem), (case["name"], p["pair"])
            n += 1
    assert n > 50


def test_planted_refusals_give_their_status():
    case, pairs, want = EM.planted()
    got = mirror(case, pairs, ret=np.zeros(2, np.int32))
    assert got.pair_status.tolist() == want
    assert got.first_layout.tolist() == [0, 1] + [1] * 9 + [2]
    assert np.array_equal(got.layouts[0:1]["total_len"], got.layouts[1:2]["total_len"]) and got.members.size == 4
    refused = np.asarray(want) != SR.SR_EDGE_OK
    assert (got.subreads[refused].view(np.int32) == -1).all()
    assert (got.subreads[~refused]["index1"] >= 0).all()


def test_min_clique_size_zero_is_refused():
    case, pairs, _ = EM.planted()
    edges, out_off, _, _ = EM.csr(case["V"], case["edges_in"])
    with pytest.raises(Exception, match="filter_subreads"):
        host.sr_edge_merge_layouts(edges, out_off, EM.random_reads(case["reads"], 3), pairs, case["vertex_read"], case["vertex_fwd"], min_clique_size=0)


ABI_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "hcsr.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(hc_sr_subread_info), sizeof(hc_merge_pairs_stats), offsetof(hc_sr_subread_info, startpos1),
           offsetof(hc_sr_subread_info, index2));
    hc_edge_rec e[1] = {{0}};
    e[0].v1 = 0; e[0].v2 = 1; e[0].read1 = 0; e[0].read2 = 1; e[0].pos1 = 7; e[0].ord = '-';
    uint64_t out_off[3] = {0, 1, 1}, seq_off[3] = {0, 30, 70}, first[3], n = 0;
    uint32_t rfs[3] = {0, 1, 2}, pairs[2], vread[2] = {0, 1}, st[1];
    uint8_t fwd[2] = {1, 0};
    if (hc_host_graph_merge_pairs(e, out_off, 2, pairs, 1, &n) != HC_OK || n != 1 || pairs[0] != 0 || pairs[1] != 1) return 2;
    hc_sr_settings s = {0.99, 2, 0, 0, 1};
    hc_sr_layout lay[2];
    hc_sr_member mem[6];
    hc_sr_subread_info sub[2];
    int32_t ret[1] = {3};
    if (hc_host_sr_edge_merge_layouts(e, out_off, 2, seq_off, rfs, 2, pairs, 1, vread, fwd, &s, st, first, lay, mem, ret, sub) != HC_OK) return 3;
    if (st[0] != HC_SR_EDGE_OK || first[1] != 1 || lay[0].n_members != 2 || lay[0].total_len != 47 || mem[1].pos != 7 || mem[1].rev != 1) return 4;
    if (sub[0].startpos1 != 3 || sub[0].index1 != 0 || sub[1].index1 != 4 || sub[1].startpos1 != 0 || sub[1].index2 != -1) return 5;
    return 0;
}
"""


def test_struct_sizes_through_the_abi():
    """A plain C program against the installed header and library: the struct sizes and one pair through both host calls."""
    lib_dir = os.path.join(ROOT, "haploconduct_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi")
        open(src, "w").write(ABI_SRC)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", lib_dir, "-lhcedge",
                        "-Wl,-rpath," + lib_dir], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.returncode
    assert r.stdout.split() == ["16", "24", "4", "8"]
    assert SR.SR_SUBREAD_DTYPE.itemsize == 16 and SR.SR_SUBREAD_DTYPE.fields["index2"][1] == 8
