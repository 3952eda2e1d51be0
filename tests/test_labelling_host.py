"""OverlapGraph::vertexLabellingHeuristic on the host (hc_host_graph_label_vertices, no device): the mirror against the reference's own
output on every case of tests/golden/labelling.json, field for field; the private generator against the platform's srand / rand and
the golden permutations; and a restatement of the cited lines in Python (tests/_labelling.py) against the mirror on seeded random
graphs, consistent and not."""
import ctypes as C
import ctypes.util
import hashlib

import numpy as np
import pytest

from haploconduct_amd import _native as N
from tests import _labelling as L

CASES = L.load()["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_equals_the_reference(case):
    g = L.graph(case["V"], case["edges"])
    (edges, out_off, in_nodes, in_off), fwd, counts = L.mirror(g, case["flags"], case["n_reads"])
    assert L.golden_rows(edges) == case["out"]
    assert out_off.tolist() == case["out_off"] and in_off.tolist() == case["in_off"] and in_nodes.tolist() == case["in_nodes"]
    assert fwd.tolist() == case["orientations"]
    assert counts["edges_before"] == len(case["edges"]) and counts["edges_after"] == case["edge_count"]
    assert counts["conflict_count"] == case["conflict_count"] == len(case["deleted"])
    assert counts["tries"] == case["tries"] and counts["n_moved"] == len(case["moved"])
    assert (counts["status"], counts["bad_v"], counts["bad_pos"]) == (case["status"], case["bad_v"], case["bad_pos"])
    # the records that carry no orientation travel untouched
    for f in ("score", "mismatch_rate", "len0", "len1", "len2"):
        assert np.array_equal(edges[f], g[0][f][edges["perc"]])
    # the best try's moved copies stand behind their new lists' own records, by (old source, old position): the order of the moves
    moved_rows = [r for r in case["out"] if r[0] != case["edges"][r[11]]["v1"]]
    assert sorted(map(tuple, moved_rows)) == sorted(map(tuple, case["moved"]))


def test_inconsistent_components_are_counted():
    by = {c["name"]: c for c in CASES}
    for name, comps, odd in (("triangle_one_odd", 1, 1), ("odd_next_to_consistent", 2, 1), ("isolated_only", 4, 0), ("two_chains_id_tie", 4, 0)):
        c = by[name]
        _, _, counts = L.mirror(L.graph(c["V"], c["edges"]))
        assert (counts["n_components"], counts["n_inconsistent"]) == (comps, odd), name


def test_repeated_record_is_refused_untouched():
    E = [L.load()["cases"][0]["edges"][0]]
    edges = [dict(E[0], v1=0, v2=1), dict(E[0], v1=2, v2=3), dict(E[0], v1=2, v2=4), dict(E[0], v1=2, v2=3, pos1=1), dict(E[0], v1=2, v2=3)]
    g = L.graph(5, edges)
    got, fwd, counts = L.mirror(g)
    assert (counts["status"], counts["bad_v"], counts["bad_pos"]) == (2, 2, 2)
    assert L.same_graph(got, g) and counts["tries"] == 0 and fwd.tolist() == [1] * 5


def test_generator_equals_the_platforms_rand():
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.rand.restype = C.c_int
    out = np.zeros(10000, np.int32)
    for seed in range(1, 101):
        N.check(N.lib.hc_host_label_rand(seed, out.ctypes.data, out.size), "hc_host_label_rand")
        libc.srand(seed)
        assert out.tolist() == [libc.rand() for _ in range(out.size)], seed


def test_shuffle_equals_the_golden_permutations():
    perm = np.zeros(256, np.uint32)
    lengths, digests, seed1 = L.golden_shuffles()
    assert lengths == list(range(2, 71)) + [200] and sorted(digests) == list(range(1, 101))
    for seed, want in digests.items():
        got, restated = bytearray(), bytearray()
        for n in lengths:
            N.check(N.lib.hc_host_label_shuffle(seed, perm.ctypes.data, n), "hc_host_label_shuffle")
            got += bytes(perm[:n].astype(np.uint8))
            if seed <= 3:  # the restatement's generator too
                items = list(range(n))
                L.random_shuffle(seed, items)
                restated += bytes(items)
        assert hashlib.sha256(bytes(got)).hexdigest() == want, seed
        assert seed > 3 or restated == got, seed
        assert seed != 1 or bytes(got) == seed1


@pytest.mark.parametrize("V,n_edges,n_odd,n_comp,seed", [(40, 90, 0, 3, 1), (60, 150, 4, 2, 2), (300, 700, 0, 5, 3), (300, 900, 6, 4, 4), (120, 200, 1, 1, 5),
                                                         (25, 24, 0, 25, 6)])
def test_restatement_agrees_with_the_mirror(V, n_edges, n_odd, n_comp, seed):
    rng = np.random.default_rng(seed)
    g = L.graph(V, L.random_edges(rng, V, n_edges, n_odd, n_comp))
    (edges, out_off, in_nodes, in_off), fwd, counts = L.mirror(g)
    r = L.Restated(g)
    opt = r.run()
    assert L.golden_rows(edges) == r.rows()
    assert in_nodes.tolist() == r.in_lists() and fwd.tolist() == opt
    assert (counts["tries"], counts["conflict_count"]) == (r.tries, r.conflict_count)
    # an odd cycle conflicts under every labelling, and nothing else does
    assert (counts["tries"] == 100) == (counts["n_inconsistent"] > 0) == (counts["conflict_count"] > 0)
    assert (counts["n_inconsistent"] > 0) == (n_odd > 0)  # (at these densities no odd record is a bridge)
