#!/usr/bin/env python3
"""Generates tests/golden/trans_edges.json with the reference's own OverlapGraph::removeInclusions and
OverlapGraph::removeTransitiveEdges.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory:
build-owned class shells (below) around src/GraphAlgos.cpp:20-48 (removeInclusions), :746-833 (findTransEdges,
nonemptyIntersect, sortAdjLists, sortAdjOut), :938-1077 (removeTransitiveEdges) and the OverlapGraph.cpp methods they
call (addEdge :94-101, removeEdge :102-147, checkEdge :233-259, getEdgeInfo :262-284), streamed from the reference by
line range.  The probe builds each graph by addEdge calls in the order given, calls the two methods and hands back
adj_out (list order), adj_in, edge_count and inclusion_edges.  transitive_count is the last "edges kept" line that
findTransEdges prints with verbose on.  Every input edge carries a distinct pos4, so an output record is stored as the
index of the input record it equals (checked here field by field).  The vectors are data; no reference source is stored.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

SHELL_HEAD = r"""
#include <assert.h>
#include <stdint.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <iostream>
#include <list>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include "Types.h"
#include "Read.h"
#include "Edge.h"

class OverlapGraph {
public:
    unsigned int vertex_count = 0;
    unsigned int edge_count = 0;
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    ProgramSettings program_settings;
    std::vector<bool> inclusions;
    std::vector< std::vector< Edge > > inclusion_edges;
    void addEdge(Edge edge);
    Edge removeEdge(node_id_t v, node_id_t w);
    double checkEdge(node_id_t v, node_id_t w, bool reverse_allowed);
    Edge* getEdgeInfo(node_id_t v, node_id_t w, bool reverse_allowed);
    void removeInclusions();
    void removeTransitiveEdges();
    unsigned int findTransEdges(std::vector< std::list< node_id_t > > & cur_adj_in, std::vector< std::list< node_id_t > > & cur_adj_out,
                                std::vector< std::list< node_id_t > > & new_adj_in, std::vector< std::list< node_id_t > > & new_adj_out,
                                bool removeTrans);
    bool nonemptyIntersect(std::list< node_id_t > & list1, std::list< node_id_t > & list2);
    std::vector< std::list< node_id_t > > sortAdjLists(std::vector< std::list< node_id_t > > & input_lists);
    std::vector< std::list< node_id_t > > sortAdjOut(std::vector< std::list< Edge > > & input_lists);
};
"""

SHELL_TAIL = r"""
}  // end of removeTransitiveEdges

struct frag_edge {
    double score, mismatch_rate;
    int32_t pos1, pos2, pos3, pos4;
    uint8_t ori1, ori2, ord, pad;
    uint32_t pad2;
    uint64_t v1, v2;
    int32_t perc, len0, len1, len2;
};

static frag_edge flat(Edge e) {
    frag_edge o;
    memset(&o, 0, sizeof o);
    o.score = e.get_score();
    o.mismatch_rate = e.get_mismatch_rate();
    o.pos1 = e.get_pos(1);
    o.pos2 = e.get_pos(2);
    o.pos3 = e.get_extra_pos(1);
    o.pos4 = e.get_extra_pos(2);
    o.ori1 = e.get_ori(1);
    o.ori2 = e.get_ori(2);
    o.ord = (uint8_t)e.get_ord();
    o.v1 = e.get_vertex(1);
    o.v2 = e.get_vertex(2);
    o.perc = e.get_perc();
    o.len0 = e.get_len(0);
    o.len1 = e.get_len(1);
    o.len2 = e.get_len(2);
    return o;
}

// stats: edge_count, transitive_count (-1 = not run), n_groups, group edges, seconds of removeTransitiveEdges
extern "C" int trans_probe(const frag_edge* in, uint64_t n, uint32_t V, const uint8_t* incl, int do_incl, int remove_trans, int branch_reduction,
                           frag_edge* out, uint64_t* out_off, uint64_t* in_off, uint64_t* in_nodes, uint64_t* group_vertex, uint64_t* group_off,
                           frag_edge* group_edges, double* stats) {
    std::vector<Read> reads;
    reads.reserve(V);
    for (uint32_t v = 0; v < V; v++) reads.push_back(Read(false, false, v, std::string(100, 'A'), "", std::string(100, 'I'), ""));
    OverlapGraph g;
    g.program_settings = ProgramSettings();
    g.program_settings.edge_threshold = 0;
    g.program_settings.merge_contigs = 0;
    g.program_settings.verbose = true;
    g.program_settings.remove_trans = remove_trans;
    g.program_settings.branch_reduction = branch_reduction != 0;
    g.vertex_count = V;
    g.adj_out.assign(V, std::list<Edge>());
    g.adj_in.assign(V, std::list<node_id_t>());
    g.inclusions.assign(V, false);
    for (uint32_t v = 0; v < V; v++) g.inclusions[v] = incl[v] != 0;
    for (uint64_t i = 0; i < n; i++) {
        const frag_edge& r = in[i];
        if (r.v1 >= V || r.v2 >= V) return 1;
        Edge e(r.score, r.pos1, r.pos2, r.ori1 != 0, r.ori2 != 0, std::string(1, (char)r.ord), &reads[r.v1], &reads[r.v2]);
        e.set_vertices(r.v1, r.v2);
        e.set_extra_pos(r.pos3, r.pos4);
        e.set_perc(r.perc);
        e.set_len(r.len1, r.len2);
        e.set_mismatch(r.mismatch_rate);
        g.addEdge(e);
    }
    std::ostringstream captured;
    std::streambuf* old = std::cout.rdbuf(captured.rdbuf());
    if (do_incl) g.removeInclusions();
    std::ostringstream trans_log;
    std::cout.rdbuf(trans_log.rdbuf());
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    g.removeTransitiveEdges();
    clock_gettime(CLOCK_MONOTONIC, &t1);
    std::cout.rdbuf(old);
    double kept = -1;
    std::istringstream lines(trans_log.str());
    for (std::string line; std::getline(lines, line);) {
        size_t p = line.find(" edges kept");
        if (p != std::string::npos) kept = atof(line.substr(0, p).c_str());
    }
    uint64_t k = 0;
    for (uint32_t v = 0; v < V; v++) {
        out_off[v] = k;
        for (const Edge& e : g.adj_out[v]) out[k++] = flat(e);
    }
    out_off[V] = k;
    uint64_t m = 0;
    for (uint32_t v = 0; v < V; v++) {
        in_off[v] = m;
        for (node_id_t x : g.adj_in[v]) in_nodes[m++] = x;
    }
    in_off[V] = m;
    uint64_t q = 0, gi = 0;
    for (uint32_t v = 0; v < V && do_incl; v++)
        if (g.inclusions[v]) group_vertex[gi++] = v;
    for (size_t k = 0; k < g.inclusion_edges.size(); k++) {
        group_off[k] = q;
        for (const Edge& e : g.inclusion_edges[k]) group_edges[q++] = flat(e);
    }
    group_off[g.inclusion_edges.size()] = q;
    if (gi != g.inclusion_edges.size()) return 2;
    stats[0] = g.edge_count;
    stats[1] = kept;
    stats[2] = (double)gi;
    stats[3] = (double)q;
    stats[4] = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    return 0;
}
"""

RANGES = [("GraphAlgos.cpp", 20, 48), ("GraphAlgos.cpp", 746, 833), ("OverlapGraph.cpp", 94, 147), ("OverlapGraph.cpp", 233, 284),
          ("GraphAlgos.cpp", 938, 1077)]


class FragEdge(C.Structure):
    _fields_ = [("score", C.c_double), ("mismatch_rate", C.c_double), ("pos1", C.c_int32), ("pos2", C.c_int32), ("pos3", C.c_int32),
                ("pos4", C.c_int32), ("ori1", C.c_uint8), ("ori2", C.c_uint8), ("ord", C.c_uint8), ("pad", C.c_uint8), ("pad2", C.c_uint32),
                ("v1", C.c_uint64), ("v2", C.c_uint64), ("perc", C.c_int32), ("len0", C.c_int32), ("len1", C.c_int32), ("len2", C.c_int32)]


def build_probe(tmp, flags=("-O2",)):
    src = [SHELL_HEAD]
    for f, a, b in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n")
    src.append(SHELL_TAIL)
    lib = os.path.join(tmp, "libtransprobe.so")
    subprocess.run(["g++", *flags, "-std=c++14", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib], input="".join(src), text=True,
                   check=True)
    dll = C.CDLL(lib)
    dll.trans_probe.restype = C.c_int
    dll.trans_probe.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    return dll


def to_struct(e, k):
    # e: [v1, v2, len1, len2, ori1, ori2, ord, score_code]; pos4 = k makes every record distinct
    return FragEdge([1.0, 0.99, 0.97][e[7]], [0.0, 0.01, -1.0][e[7]], 5 + e[2] % 7, 0, -3, k, e[4], e[5], e[6], 0, 0, e[0], e[1],
                    [100, 77, 91][e[7]], e[2] + e[3], e[2], e[3])


def run(dll, V, edges, incl, do_incl, rt, br):
    n = len(edges)
    arr = (FragEdge * max(n, 1))()
    for k, e in enumerate(edges):
        arr[k] = to_struct(e, k)
    out = (FragEdge * max(n, 1))()
    gedges = (FragEdge * max(2 * n, 1))()
    out_off, in_off = np.zeros(V + 1, np.uint64), np.zeros(V + 1, np.uint64)
    in_nodes = np.zeros(max(n, 1), np.uint64)
    gv, goff = np.zeros(V + 1, np.uint64), np.zeros(V + 1, np.uint64)
    stats = np.zeros(5, np.float64)
    inc = np.ascontiguousarray(incl, dtype=np.uint8) if V else np.zeros(1, np.uint8)
    rc = dll.trans_probe(arr, n, V, inc.ctypes.data, do_incl, rt, br, out, out_off.ctypes.data, in_off.ctypes.data, in_nodes.ctypes.data,
                         gv.ctypes.data, goff.ctypes.data, gedges, stats.ctypes.data)
    assert rc == 0, rc

    def idx(o):
        k = o.pos4
        ref = arr[k]
        assert all(getattr(o, f) == getattr(ref, f) for f, _ in FragEdge._fields_), "record does not equal its input"
        return k

    m = int(out_off[V])
    ng, nq = int(stats[2]), int(stats[3])
    return dict(remove_trans=rt, branch_reduction=br, inclusions=do_incl, edge_count=int(stats[0]), transitive_count=int(stats[1]),
                out=[idx(o) for o in out[:m]], out_off=out_off.tolist(), in_off=in_off.tolist(), in_nodes=in_nodes[:int(in_off[V])].tolist(),
                group_vertex=gv[:ng].tolist(), group_off=goff[:ng + 1].tolist(), group_edges=[idx(o) for o in gedges[:nq]]), stats[4]


def edge(rng, a, b, l1=None, o=None):
    o1, o2 = o if o else (1, 1)
    return [a, b, l1 if l1 is not None else rng.choice([40, 60, 80, 100, 120]), rng.choice([0, 0, 30]), o1, o2, ord(rng.choice("-12")),
            rng.randrange(3)]


def interval_graph(seed, V, reach, jitter=0.0):
    """Reads tiled along a genome: read i overlaps every read that starts within `reach` after it (out-lists in a shuffled order)."""
    rng = random.Random(seed)
    pos = sorted(rng.randrange(V * 10) for _ in range(V))
    edges = []
    for i in range(V):
        lst = [edge(rng, i, j, l1=reach + 20 - (pos[j] - pos[i])) for j in range(i + 1, V) if pos[j] - pos[i] < reach and rng.random() >= jitter]
        rng.shuffle(lst)
        edges += lst
    return edges


def sparse_graph(seed, V, n):
    rng = random.Random(seed)
    edges = []
    while len(edges) < n:
        a, b = rng.randrange(V), rng.randrange(V)
        if a != b:
            edges.append(edge(rng, a, b))
    return edges


def hub_graph(seed, V, hub_out, hub_in):
    """An interval backbone plus hubs: `hub_out` gets an edge to every other vertex, every vertex gets one into `hub_in`."""
    rng = random.Random(seed)
    edges = interval_graph(seed, V, 25, jitter=0.3)
    edges += [edge(rng, hub_out, j) for j in range(V) if j != hub_out and rng.random() < 0.9]
    edges += [edge(rng, j, hub_in) for j in range(V) if j != hub_in and rng.random() < 0.9]
    rng.shuffle(edges)
    return edges


def repeated_graph(seed, V):
    """Repeated targets: the two orientation classes of one pair (one list of <= 16, one of > 16 entries, one of > 100)."""
    rng = random.Random(seed)
    edges = interval_graph(seed, V, 40, jitter=0.5)
    extra = []
    for (u, deg) in ((0, 12), (1, 30), (2, 120)):
        targets = rng.sample(range(3, V), min(deg, V - 3))
        for t in targets:
            extra.append(edge(rng, u, t, o=(1, 1)))
            if rng.random() < 0.5:
                extra.append(edge(rng, u, t, l1=rng.choice([40, 60, 80, 100, 120]), o=(1, 0)))
            if rng.random() < 0.3:
                extra.append(edge(rng, t, u, o=(0, 1)))
    rng.shuffle(extra)
    return edges + extra


def duplicates_graph(seed, n_reads, reach):
    """add_duplicates style: vertices [0, n) and their reverse complements [n, 2n), every edge mirrored between the copies."""
    rng = random.Random(seed)
    base = interval_graph(seed, n_reads, reach, jitter=0.2)
    mirrored = []
    for e in base:
        m = list(e)
        m[0], m[1] = e[1] + n_reads, e[0] + n_reads
        m[4], m[5] = 1 - e[5], 1 - e[4]
        mirrored.append(m)
    out = base + mirrored
    rng.shuffle(out)
    return out


def cases():
    yield "interval", 60, interval_graph(1, 60, 30), (1, 2, 3)
    yield "interval_dense", 40, interval_graph(2, 40, 60), (1, 2)
    yield "sparse", 120, sparse_graph(3, 120, 200), (1, 2)
    yield "hubs", 130, hub_graph(4, 130, 7, 11), (1, 2, 3)
    yield "repeated", 150, repeated_graph(5, 150), (1, 2, 3)
    yield "duplicates", 60, duplicates_graph(6, 30, 40), (1, 2)
    yield "isolated", 30, [e for e in interval_graph(7, 30, 35) if e[0] % 5 and e[1] % 5], (1, 3)
    yield "empty", 4, [], (1,)


def main():
    out_cases, timing = [], []
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        for name, V, edges, rts in cases():
            rng = random.Random(len(name))
            incl = [1 if rng.random() < 0.06 else 0 for _ in range(V)]
            variants = []
            for rt in rts:
                for br in (0, 1):
                    for do_incl in (0, 1):
                        if rt > 1 and br == 1 and do_incl:
                            continue  # branch reduction only acts with remove_trans == 1
                        r, _ = run(dll, V, edges, incl, do_incl, rt, br)
                        variants.append(r)
            print(f"{name}: V={V} edges={len(edges)} variants={len(variants)}")
            out_cases.append(dict(name=name, V=V, edges_in=edges, incl=incl, variants=variants))
        # the reference's own removeTransitiveEdges on a larger interval graph, for the timing record (not stored as a case)
        big = interval_graph(9, 20000, 640)
        r, secs = run(dll, 20000, big, [0] * 20000, 0, 1, 0)
        timing.append(dict(V=20000, edges=len(big), remove_trans=1, seconds=float(secs)))
        print("timing", timing[-1])
    fields = ["v1", "v2", "len1", "len2", "ori1", "ori2", "ord", "code"]
    doc = dict(note="OverlapGraph::removeInclusions + removeTransitiveEdges of the reference (GraphAlgos.cpp:20-48, 746-833, 938-1077) "
                    "through a probe; edges_in = addEdge order, one record per entry: " + ",".join(fields) +
                    "; the full record of input k: score/perc/mismatch by code ([1.0,0.99,0.97], [100,77,91], [0.0,0.01,-1.0]), "
                    "pos1 = 5 + len1 % 7, pos2 = 0, pos3 = -3, pos4 = k, len0 = len1 + len2.  out / group_edges: input indices in list order.",
               cases=out_cases)
    path = os.path.join(ROOT, "tests", "golden", "trans_edges.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(timing, f)


if __name__ == "__main__":
    main()
