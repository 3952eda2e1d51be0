#!/usr/bin/env python3
"""Generates tests/golden/cycles.json with the reference's own OverlapGraph::sortEdges and cycleRemovalHeuristic.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory: build-owned
declaration-only shells (below) around src/GraphAlgos.cpp:150-176 (sortVerticesByIndegree), :352-541 (dfs_helper, findCycles,
cycleRemovalHeuristic) and src/OverlapGraph.cpp:104-147 (removeEdge), :548-562 (reportCycle), :722-764 (sortEdges), streamed from the
reference by line range and never stored, with the genuine Types.h, Read.h and Edge.h.  A std::vector<bool> stands for the bitsets
(construction with a size, indexing and assignment are all that is used).  PATH is a temporary directory, from which cycles.txt is
read back.  Every input record carries its index as perc, so lists are recorded as record indices.

Per case: the input records and read lengths; the lists after sortEdges; findCycles(t) for t = 1 .. 20 called directly; and, after
cycleRemovalHeuristic on a fresh graph for both values of remove_edges: both lists, branching_edges, backedge_count and the bytes of
cycles.txt (null: no file).  The vectors are data; no reference source is stored.
"""
import ctypes as C
import json
import os
import random
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

SHELL_HEAD = r"""
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <list>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include "Types.h"
#include "Read.h"
#include "Edge.h"

namespace boost {
template <class Block = unsigned long>
struct dynamic_bitset : std::vector<bool> {
    dynamic_bitset() {}
    explicit dynamic_bitset(size_t n) : std::vector<bool>(n, false) {}
};
}

class OverlapGraph {
public:
    unsigned int vertex_count = 0;
    unsigned int edge_count = 0;
    unsigned int graph_depth = 0;
    unsigned int backedge_count = 0;
    std::string PATH;
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    std::list< Edge > branching_edges;
    ProgramSettings program_settings;
    Edge removeEdge(node_id_t v, node_id_t w);
    void reportCycle(node_id_t u, node_id_t v, bool remove);
    void sortEdges();
    std::vector< node_id_t > sortVerticesByIndegree();
    void dfs_helper(node_id_t parent, node_id_t node, boost::dynamic_bitset<> &marked, boost::dynamic_bitset<> &visited, std::vector<node_id_t>& path, std::set< std::pair< node_id_t, node_id_t > >& backedge_vec, int randomize);
    std::set< std::pair< node_id_t, node_id_t > > findCycles(int randomize);
    void cycleRemovalHeuristic(bool remove_edges);
};
"""

SHELL_TAIL = r"""
struct probe_edge {
    double score, mismatch_rate;
    int32_t pos1, len1;
    uint32_t v1, v2;
};

static void dump(OverlapGraph& g, uint32_t V, uint32_t* out, uint64_t* out_off, uint32_t* in_nodes, uint64_t* in_off) {
    uint64_t k = 0, m = 0;
    for (uint32_t v = 0; v < V; v++) {
        out_off[v] = k;
        for (Edge& e : g.adj_out[v]) out[k++] = (uint32_t)e.get_perc();
        in_off[v] = m;
        for (node_id_t x : g.adj_in[v]) in_nodes[m++] = (uint32_t)x;
    }
    out_off[V] = k;
    in_off[V] = m;
}

// sets: the 20 sets back to back as (u, v), set_off: 21 offsets in pairs.  stats: edge_count, backedge_count, |branching_edges|.
extern "C" int cycles_probe(const probe_edge* in, uint64_t n, uint32_t V, const uint32_t* len_by_read, int remove_edges, const char* path,
                            uint32_t* sorted_out, uint64_t* sorted_out_off, uint32_t* sorted_in, uint64_t* sorted_in_off, uint32_t* sets,
                            uint64_t sets_cap, uint64_t* set_off, uint32_t* out, uint64_t* out_off, uint32_t* in_nodes, uint64_t* in_off,
                            uint32_t* branching, uint64_t* stats) {
    std::vector<Read> reads;
    reads.reserve(V);
    for (uint32_t r = 0; r < V; r++)
        reads.push_back(Read(false, false, r, std::string(len_by_read[r], 'A'), std::string(), std::string(len_by_read[r], 'I'), std::string()));
    OverlapGraph g;
    g.program_settings = ProgramSettings();
    g.program_settings.verbose = false;
    g.PATH = path;
    g.vertex_count = V;
    g.adj_out.assign(V, std::list<Edge>());
    g.adj_in.assign(V, std::list<node_id_t>());
    for (uint64_t i = 0; i < n; i++) {
        const probe_edge& r = in[i];
        if (r.v1 >= V || r.v2 >= V) return 1;
        Edge e(r.score, r.pos1, 0, true, true, std::string("-"), &reads[r.v1], &reads[r.v2]);
        e.set_vertices(r.v1, r.v2);
        e.set_perc((int)i);
        e.set_len(r.len1, 0);
        e.set_mismatch(r.mismatch_rate);
        g.adj_out[r.v1].push_back(e);  // addEdge, src/OverlapGraph.cpp:94-101
        g.adj_in[r.v2].push_back(r.v1);
        g.edge_count++;
    }
    g.sortEdges();
    dump(g, V, sorted_out, sorted_out_off, sorted_in, sorted_in_off);
    uint64_t k = 0;
    for (int t = 1; t <= 20; t++) {
        set_off[t - 1] = k;
        const std::set< std::pair< node_id_t, node_id_t > > s = g.findCycles(t);
        for (const auto& p : s) {
            if (k >= sets_cap) return 2;
            sets[2 * k] = (uint32_t)p.first, sets[2 * k + 1] = (uint32_t)p.second;
            k++;
        }
    }
    set_off[20] = k;
    g.cycleRemovalHeuristic(remove_edges != 0);
    dump(g, V, out, out_off, in_nodes, in_off);
    if (out_off[V] != g.edge_count) return 3;
    uint64_t b = 0;
    for (Edge& e : g.branching_edges) branching[b++] = (uint32_t)e.get_perc();
    stats[0] = g.edge_count, stats[1] = g.backedge_count, stats[2] = b;
    return 0;
}
"""

RANGES = [("GraphAlgos.cpp", 150, 176), ("GraphAlgos.cpp", 352, 541), ("OverlapGraph.cpp", 104, 147), ("OverlapGraph.cpp", 548, 562),
          ("OverlapGraph.cpp", 722, 764)]
EDGE_FIELDS = ["v1", "v2", "pos1", "len1", "score", "mismatch_rate"]  # an input record; read1 = v1, read2 = v2, len0 = len1


class ProbeEdge(C.Structure):
    _fields_ = [("score", C.c_double), ("mismatch_rate", C.c_double), ("pos1", C.c_int32), ("len1", C.c_int32), ("v1", C.c_uint32), ("v2", C.c_uint32)]


def build_probe(tmp):
    src = [SHELL_HEAD]
    for f, a, b in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n")
    src.append(SHELL_TAIL)
    lib = os.path.join(tmp, "libcyclesprobe.so")
    subprocess.run(["g++", "-O2", "-Wno-deprecated-declarations", "-std=c++14", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib],
                   input="".join(src), text=True, check=True)
    dll = C.CDLL(lib)
    dll.cycles_probe.restype = C.c_int
    dll.cycles_probe.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_char_p] + [C.c_void_p] * 5 + [C.c_uint64] + [C.c_void_p] * 7
    return dll


def run(dll, tmp, V, lens, edges, remove_edges):
    n = len(edges)
    arr = (ProbeEdge * max(n, 1))()
    for k, e in enumerate(edges):
        arr[k] = ProbeEdge(e["score"], e["mismatch_rate"], e["pos1"], e["len1"], e["v1"], e["v2"])
    L = np.asarray(lens, np.uint32)
    n1 = max(n, 1)
    so, si, out, inn, br = (np.zeros(n1, np.uint32) for _ in range(5))
    soo, sio, oo, io = (np.zeros(V + 1, np.uint64) for _ in range(4))
    sets, set_off, stats = np.zeros(2 * 20 * n1, np.uint32), np.zeros(21, np.uint64), np.zeros(3, np.uint64)
    d = tempfile.mkdtemp(dir=tmp) + "/"
    rc = dll.cycles_probe(arr, n, V, L.ctypes.data, int(remove_edges), d.encode(), so.ctypes.data, soo.ctypes.data, si.ctypes.data, sio.ctypes.data,
                          sets.ctypes.data, 20 * n1, set_off.ctypes.data, out.ctypes.data, oo.ctypes.data, inn.ctypes.data, io.ctypes.data, br.ctypes.data,
                          stats.ctypes.data)
    assert rc == 0, rc
    txt = None
    if os.path.exists(d + "cycles.txt"):
        with open(d + "cycles.txt") as f:
            txt = f.read()
    m = int(stats[0])
    try_sets = [sets[2 * int(set_off[t]):2 * int(set_off[t + 1])].reshape(-1, 2).tolist() for t in range(20)]
    return dict(sorted_out=so[:n].tolist(), sorted_out_off=soo.tolist(), sorted_in=si[:n].tolist(), sorted_in_off=sio.tolist(), sets=try_sets,
                after=dict(out=out[:m].tolist(), out_off=oo.tolist(), in_nodes=inn[:m].tolist(), in_off=io.tolist(), branching=br[:int(stats[2])].tolist(),
                           backedge_count=int(stats[1]), cycles_txt=txt))


def edge(v1, v2, pos1=5, len1=30, score=1.0, mm=0.25):
    return dict(v1=v1, v2=v2, pos1=pos1, len1=len1, score=score, mismatch_rate=mm)


def random_graph(rng, V, n_edges, acyclic=False, first=0, neg=False):
    """Random digraph on [first, first + V): keys drawn from few values so that ties are common; acyclic: every record ascends."""
    out = []
    for _ in range(n_edges):
        a, b = rng.randrange(V), rng.randrange(V)
        if a == b:
            continue
        if acyclic and a > b:
            a, b = b, a
        out.append(edge(first + a, first + b, pos1=rng.randrange(-6 if neg else 0, 7), len1=rng.randrange(20, 40), score=rng.randrange(1, 9) / 8.0,
                        mm=rng.randrange(0, 9) / 64.0))
    return out


def hub_on_cycle(first=0, deg=20):
    """first has `deg` out-records to distinct targets, one of which leads back to it; keys distinct, so no list is fully tied."""
    out = [edge(first, first + 1 + t, pos1=(7 * t) % deg, len1=20 + t, score=(1 + (3 * t) % deg) / 32.0, mm=((5 * t) % deg) / 64.0) for t in range(deg)]
    out.append(edge(first + 3, first, pos1=2))
    out.append(edge(first + 9, first + 3, pos1=1))
    return deg + 1, out


def search(dll, tmp, what, want, make):
    for seed in range(1, 2000):
        V, lens, es = make(random.Random(seed))
        if want(run(dll, tmp, V, lens, es, 1)):
            return V, lens, es
    raise SystemExit(f"no seed gives a graph with {what}")


def sizes(r):
    return [len(s) for s in r["sets"]]


def first_min(r):
    z = sizes(r)
    return z.index(min(z))


def cases(dll, tmp):
    rng = random.Random(20240607)
    cs = []

    def lens_for(V, r=rng):
        return [r.randrange(60, 140) for _ in range(V)]

    cs.append(("acyclic", 40, lens_for(40), random_graph(rng, 40, 90, acyclic=True)))
    cs.append(("isolated_only", 3, lens_for(3), []))
    cs.append(("ring", 5, lens_for(5), [edge(k, (k + 1) % 5, pos1=k) for k in range(5)]))
    cs.append(("self_loop", 4, lens_for(4), [edge(0, 1), edge(1, 1, pos1=2), edge(1, 2), edge(2, 3)]))
    cs.append(("two_cycle", 3, lens_for(3), [edge(0, 1), edge(1, 0, pos1=3), edge(1, 2)]))
    cs.append(("repeated_pair", 3, lens_for(3), [edge(0, 1, len1=30), edge(0, 1, len1=25, score=0.5), edge(1, 0, len1=30), edge(1, 0, len1=22, score=0.25), edge(1, 2)]))

    def small(r):
        V = 12
        return V, lens_for(V, r), random_graph(r, V, 34)

    cs.append(("best_not_first",) + search(dll, tmp, "a best try that is not try 1", lambda r: first_min(r) != 0, small))

    def tie_want(r):
        z, f = sizes(r), first_min(r)
        return z[f] > 0 and any(z[t] == z[f] and r["sets"][t] != r["sets"][f] for t in range(f + 1, 20))

    cs.append(("tie_earlier_wins",) + search(dll, tmp, "a tie in size between different sets", tie_want, small))
    # two cyclic components among acyclic ones
    es = random_graph(rng, 10, 20, acyclic=True) + [edge(10 + k, 10 + (k + 1) % 4, pos1=k) for k in range(4)] + random_graph(rng, 8, 14, acyclic=True, first=14)
    es += random_graph(rng, 7, 18, first=22) + random_graph(rng, 6, 9, acyclic=True, first=29)
    cs.append(("two_cyclic_among_acyclic", 36, lens_for(36), es))
    V, es = hub_on_cycle()
    cs.append(("hub_on_cycle", V, lens_for(V), es))
    cs.append(("negative_pos1", 14, lens_for(14), random_graph(rng, 14, 40, neg=True)))
    # equal keys decided by the target: one key value in every column
    cs.append(("keys_all_equal", 8, [100] * 8, [edge(a, b) for a, b in ((0, 3), (0, 2), (0, 1), (3, 0), (2, 3), (1, 2), (2, 0), (3, 5), (5, 6), (6, 7), (7, 5), (4, 0))]))
    cs.append(("zero_signs", 5, lens_for(5), [edge(0, 2, score=0.0, mm=-0.0), edge(0, 1, score=-0.0, mm=0.0), edge(1, 0, score=0.0, mm=0.0), edge(2, 0, score=-0.0, mm=-0.0),
                                              edge(1, 3, score=0.5, mm=-1.0), edge(3, 1, score=0.0, mm=0.125), edge(3, 4)]))
    return cs


def check_coverage(by):
    def applied(c):
        return [[int(x) for x in ln.split("\t")] for ln in c["remove"]["cycles_txt"].splitlines()]

    for c in by.values():  # what holds for every case, from the reference's output alone
        z, f = sizes(c), first_min(c)
        for key in ("remove", "keep"):
            a = c[key]
            assert a["backedge_count"] == z[f]
            assert (a["cycles_txt"] is None) == (z[f] == 0)
            if z[f]:
                assert [[int(x) for x in ln.split("\t")] for ln in a["cycles_txt"].splitlines()] == c["sets"][f], c["name"]
        assert c["keep"]["out"] == c["sorted_out"] and c["keep"]["in_nodes"] == c["sorted_in"] and not c["keep"]["branching"]
        assert len(c["remove"]["branching"]) == z[f] and len(c["remove"]["out"]) == len(c["edges"]) - z[f]
    c = by["acyclic"]
    assert sizes(c)[0] == 0 and c["remove"]["cycles_txt"] is None and c["remove"]["out"] == c["sorted_out"], "acyclic: one try, no file"
    assert first_min(by["best_not_first"]) != 0
    c = by["tie_earlier_wins"]
    z, f = sizes(c), first_min(c)
    assert any(z[t] == z[f] and c["sets"][t] != c["sets"][f] for t in range(f + 1, 20)) and applied(c) == c["sets"][f]
    assert any(u == v for u, v in applied(by["self_loop"]))
    c = by["two_cycle"]
    assert applied(c) in ([[0, 1]], [[1, 0]])
    c = by["repeated_pair"]
    (u, v), = applied(c)
    left = [c["edges"][k] for k in c["remove"]["out"]]
    assert sum(e["v1"] == u and e["v2"] == v for e in left) == 1, "repeated pair: one record stays"
    gone = c["edges"][c["remove"]["branching"][0]]
    first = next(k for k in c["sorted_out"] if c["edges"][k]["v1"] == u and c["edges"][k]["v2"] == v)
    assert gone == c["edges"][first], "repeated pair: the first record in list order leaves"
    c = by["two_cyclic_among_acyclic"]
    comp_of = lambda v: 0 if v < 10 else 1 if v < 14 else 2 if v < 22 else 3 if v < 29 else 4
    assert {comp_of(u) for u, _ in c["sets"][0]} == {1, 3}
    c = by["hub_on_cycle"]
    assert c["sorted_out_off"][1] - c["sorted_out_off"][0] > 16 and any(0 in p for p in applied(c))
    c = by["negative_pos1"]
    assert any(e["pos1"] < 0 for e in c["edges"]) and sizes(c)[0] > 0
    c = by["keys_all_equal"]
    assert len({(e["pos1"], e["len1"], e["score"], e["mismatch_rate"]) for e in c["edges"]}) == 1 and sizes(c)[0] > 0
    assert all(c["sets"][t] == c["sets"][0] for t in range(4)), "equal keys: tries 1 - 4 are the target order"


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        by = {}
        for name, V, lens, edges in cases(dll, tmp):
            res = run(dll, tmp, V, lens, edges, 1)
            keep = run(dll, tmp, V, lens, edges, 0)
            for k in ("sorted_out", "sorted_out_off", "sorted_in", "sorted_in_off", "sets"):
                assert res[k] == keep[k]
            by[name] = dict(name=name, V=V, len_by_read=lens, edges=edges, sorted_out=res["sorted_out"], sorted_out_off=res["sorted_out_off"],
                            sorted_in=res["sorted_in"], sorted_in_off=res["sorted_in_off"], sets=res["sets"], remove=res["after"], keep=keep["after"])
        check_coverage(by)
        golden = list(by.values())
        for c in golden:  # (the input records as rows: the file stays small)
            c["edges"] = [[e[f] for f in EDGE_FIELDS] for e in c["edges"]]
        path = os.path.join(ROOT, "tests", "golden", "cycles.json")
        with open(path, "w") as f:
            json.dump(dict(edge_fields=EDGE_FIELDS, cases=golden), f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {path}: {len(golden)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
