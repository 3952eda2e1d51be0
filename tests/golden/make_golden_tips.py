#!/usr/bin/env python3
"""Generates tests/golden/tips_branches.json with the reference's own OverlapGraph::removeTips and
OverlapGraph::removeBranches.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory:
build-owned declaration-only shells (below) around src/GraphAlgos.cpp:543-637 (removeTips), :714-743 (findBranchfreeGraph,
which removeBranches calls), :746-833 (findTransEdges, nonemptyIntersect, sortAdjLists, sortAdjOut), :835-936 (removeBranches)
and src/OverlapGraph.cpp:94-147 (addEdge, removeEdge), :233-284 (checkEdge, getEdgeInfo), streamed from the reference by
line range and never stored, with the genuine Types.h, Read.h and Edge.h.  A std::vector<bool> stands for the `visited`
bitset, which is only indexed.  The probe builds each graph by addEdge calls in the order given over reads built from the
read table, runs a variant (tips / branches / tips then branches) and hands back adj_out (list order), adj_in,
edge_count, branching_edges, Read::is_tip() per read and the verbose lines, from which the counters are parsed.  Every
input edge carries a distinct pos4, so an output record is stored as the index of the input record it equals (checked
here field by field).  The vectors are data; no reference source is stored.

With an argument: also times the reference's removeTips / removeBranches on a 20 000-vertex interval graph and writes
the seconds to that file (not stored in the golden file).
"""
import ctypes as C
import json
import os
import random
import re
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
#include <map>
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
    explicit dynamic_bitset(size_t n) : std::vector<bool>(n, false) {}
};
}

class OverlapGraph {
public:
    unsigned int vertex_count = 0;
    unsigned int edge_count = 0;
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    std::vector< Edge > branching_edges;
    ProgramSettings program_settings;
    void addEdge(Edge edge);
    Edge removeEdge(node_id_t v, node_id_t w);
    double checkEdge(node_id_t v, node_id_t w, bool reverse_allowed);
    Edge* getEdgeInfo(node_id_t v, node_id_t w, bool reverse_allowed);
    void removeTips();
    void removeBranches();
    void findBranchfreeGraph(std::vector< std::list< node_id_t > > & cur_adj_in, std::vector< std::list< node_id_t > > & cur_adj_out,
                             std::set< node_id_t > & remove_in, std::set< node_id_t > & remove_out);
    unsigned int findTransEdges(std::vector< std::list< node_id_t > > & cur_adj_in, std::vector< std::list< node_id_t > > & cur_adj_out,
                                std::vector< std::list< node_id_t > > & new_adj_in, std::vector< std::list< node_id_t > > & new_adj_out,
                                bool removeTrans);
    bool nonemptyIntersect(std::list< node_id_t > & list1, std::list< node_id_t > & list2);
    std::vector< std::list< node_id_t > > sortAdjLists(std::vector< std::list< node_id_t > > & input_lists);
    std::vector< std::list< node_id_t > > sortAdjOut(std::vector< std::list< Edge > > & input_lists);
};
"""

SHELL_TAIL = r"""
struct frag_edge {
    double score, mismatch_rate;
    int32_t pos1, pos2, pos3, pos4;
    uint8_t ori1, ori2, ord, pad;
    uint32_t read1, read2, pad2;
    uint64_t v1, v2;
    int32_t perc, len0, len1, len2;
};
struct frag_read { uint32_t len1, len2; uint8_t paired, pad[3]; };

static frag_edge flat(Edge e, const Read* base) {
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
    o.read1 = (uint32_t)(e.get_read(1) - base);
    o.read2 = (uint32_t)(e.get_read(2) - base);
    o.v1 = e.get_vertex(1);
    o.v2 = e.get_vertex(2);
    o.perc = e.get_perc();
    o.len0 = e.get_len(0);
    o.len1 = e.get_len(1);
    o.len2 = e.get_len(2);
    return o;
}

// steps: bit 0 removeTips, bit 1 removeBranches (in that order).  stats: edge_count, lists of more than 16 entries with a
// repeated target when removeBranches starts, seconds of removeTips, seconds of removeBranches.  ext[2 k], ext[2 k + 1]:
// ext_len(1), ext_len(0) of input edge k.
extern "C" int tips_probe(const frag_edge* in, uint64_t n, uint32_t V, const frag_read* rd, uint32_t n_reads, uint32_t max_tip_len, int steps,
                          frag_edge* out, uint64_t* out_off, uint64_t* in_off, uint64_t* in_nodes, frag_edge* branching, uint64_t* n_branching,
                          uint8_t* is_tip, uint32_t* ext, char* log, uint64_t log_cap, double* stats) {
    std::vector<Read> reads;
    reads.reserve(n_reads);
    for (uint32_t r = 0; r < n_reads; r++)
        reads.push_back(Read(rd[r].paired != 0, false, r, std::string(rd[r].len1, 'A'), std::string(rd[r].len2, 'A'), std::string(rd[r].len1, 'I'),
                             std::string(rd[r].len2, 'I')));
    OverlapGraph g;
    g.program_settings = ProgramSettings();
    g.program_settings.edge_threshold = 0;
    g.program_settings.merge_contigs = 0;
    g.program_settings.min_overlap_perc = 0;
    g.program_settings.verbose = true;
    g.program_settings.remove_trans = 1;
    g.program_settings.max_tip_len = max_tip_len;
    g.vertex_count = V;
    g.adj_out.assign(V, std::list<Edge>());
    g.adj_in.assign(V, std::list<node_id_t>());
    for (uint64_t i = 0; i < n; i++) {
        const frag_edge& r = in[i];
        if (r.v1 >= V || r.v2 >= V || r.read1 >= n_reads || r.read2 >= n_reads) return 1;
        Edge e(r.score, r.pos1, r.pos2, r.ori1 != 0, r.ori2 != 0, std::string(1, (char)r.ord), &reads[r.read1], &reads[r.read2]);
        e.set_vertices(r.v1, r.v2);
        e.set_extra_pos(r.pos3, r.pos4);
        e.set_perc(r.perc);
        e.set_len(r.len1, r.len2);
        e.set_mismatch(r.mismatch_rate);
        ext[2 * i] = e.ext_len(true);
        ext[2 * i + 1] = e.ext_len(false);
        g.addEdge(e);
    }
    std::ostringstream captured;
    std::streambuf* old = std::cout.rdbuf(captured.rdbuf());
    struct timespec t0, t1;
    stats[1] = stats[2] = stats[3] = 0;
    if (steps & 1) {
        clock_gettime(CLOCK_MONOTONIC, &t0);
        g.removeTips();
        clock_gettime(CLOCK_MONOTONIC, &t1);
        stats[2] = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    }
    if (steps & 2) {
        for (uint32_t v = 0; v < V; v++) {
            std::vector<node_id_t> t;
            for (const Edge& e : g.adj_out[v]) t.push_back(e.get_vertex(2));
            std::sort(t.begin(), t.end());
            if (t.size() > 16 && std::adjacent_find(t.begin(), t.end()) != t.end()) stats[1] += 1;
        }
        clock_gettime(CLOCK_MONOTONIC, &t0);
        g.removeBranches();
        clock_gettime(CLOCK_MONOTONIC, &t1);
        stats[3] = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    }
    std::cout.rdbuf(old);
    const std::string text = captured.str();
    if (text.size() + 1 > log_cap) return 3;
    memcpy(log, text.c_str(), text.size() + 1);
    const Read* base = reads.data();
    uint64_t k = 0;
    for (uint32_t v = 0; v < V; v++) {
        out_off[v] = k;
        for (const Edge& e : g.adj_out[v]) out[k++] = flat(e, base);
    }
    out_off[V] = k;
    uint64_t m = 0;
    for (uint32_t v = 0; v < V; v++) {
        in_off[v] = m;
        for (node_id_t x : g.adj_in[v]) in_nodes[m++] = x;
    }
    in_off[V] = m;
    if (k != g.edge_count || m != k) return 2;
    for (size_t b = 0; b < g.branching_edges.size(); b++) branching[b] = flat(g.branching_edges[b], base);
    *n_branching = g.branching_edges.size();
    for (uint32_t r = 0; r < n_reads; r++) is_tip[r] = reads[r].is_tip() ? 1 : 0;
    stats[0] = g.edge_count;
    return 0;
}
"""

RANGES = [("GraphAlgos.cpp", 543, 637), ("GraphAlgos.cpp", 714, 743), ("GraphAlgos.cpp", 746, 833), ("GraphAlgos.cpp", 835, 936),
          ("OverlapGraph.cpp", 94, 147), ("OverlapGraph.cpp", 233, 284)]

VARIANTS = (("tips", 1), ("branches", 2), ("tips_branches", 3))


class FragEdge(C.Structure):
    _fields_ = [("score", C.c_double), ("mismatch_rate", C.c_double), ("pos1", C.c_int32), ("pos2", C.c_int32), ("pos3", C.c_int32),
                ("pos4", C.c_int32), ("ori1", C.c_uint8), ("ori2", C.c_uint8), ("ord", C.c_uint8), ("pad", C.c_uint8), ("read1", C.c_uint32),
                ("read2", C.c_uint32), ("pad2", C.c_uint32), ("v1", C.c_uint64), ("v2", C.c_uint64), ("perc", C.c_int32), ("len0", C.c_int32),
                ("len1", C.c_int32), ("len2", C.c_int32)]


class FragRead(C.Structure):
    _fields_ = [("len1", C.c_uint32), ("len2", C.c_uint32), ("paired", C.c_uint8), ("pad", C.c_uint8 * 3)]


def build_probe(tmp, flags=("-O2",)):
    src = [SHELL_HEAD]
    for f, a, b in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n")
    src.append(SHELL_TAIL)
    lib = os.path.join(tmp, "libtipsprobe.so")
    subprocess.run(["g++", *flags, "-std=c++14", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib], input="".join(src), text=True,
                   check=True)
    dll = C.CDLL(lib)
    dll.tips_probe.restype = C.c_int
    dll.tips_probe.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 9 + [C.c_uint64,
                                                                                                                                      C.c_void_p]
    return dll


FIELDS = ["v1", "v2", "read1", "read2", "pos1", "pos2", "len1", "len2", "ori1", "ori2", "ord"]


def to_struct(e, k):
    v1, v2, r1, r2, p1, p2, l1, l2, o1, o2, od = e
    return FragEdge(1.0, 0.0, p1, p2, -3, k, o1, o2, od, 0, r1, r2, 0, v1, v2, 100, l1 + l2, l1, l2)


def number(log, pattern, last=True):
    found = re.findall(pattern + r"\s*(\d+)", log)
    return int(found[-1 if last else 0]) if found else None


def run(dll, V, edges, reads, max_tip_len, steps):
    n, nr = len(edges), len(reads)
    arr = (FragEdge * max(n, 1))()
    for k, e in enumerate(edges):
        arr[k] = to_struct(e, k)
    rd = (FragRead * max(nr, 1))()
    for k, (l1, l2, p) in enumerate(reads):
        rd[k] = FragRead(l1, l2, p)
    out, branching = (FragEdge * max(n, 1))(), (FragEdge * max(n, 1))()
    out_off, in_off = np.zeros(V + 1, np.uint64), np.zeros(V + 1, np.uint64)
    in_nodes = np.zeros(max(n, 1), np.uint64)
    nb = C.c_uint64()
    is_tip = np.zeros(max(nr, 1), np.uint8)
    ext = np.zeros(2 * max(n, 1), np.uint32)
    log = C.create_string_buffer(1 << 16)
    stats = np.zeros(4, np.float64)
    rc = dll.tips_probe(arr, n, V, rd, nr, max_tip_len, steps, out, out_off.ctypes.data, in_off.ctypes.data, in_nodes.ctypes.data, branching,
                        C.byref(nb), is_tip.ctypes.data, ext.ctypes.data, log, len(log), stats.ctypes.data)
    assert rc == 0, rc

    def idx(o):
        k = o.pos4
        ref = arr[k]
        assert all(getattr(o, f) == getattr(ref, f) for f, _ in FragEdge._fields_), "record does not equal its input"
        return k

    text = log.value.decode()
    m = int(out_off[V])
    res = dict(edge_count=int(stats[0]), out=[idx(o) for o in out[:m]], out_off=out_off.tolist(), in_off=in_off.tolist(),
               in_nodes=in_nodes[:m].tolist(), branching=[idx(o) for o in branching[:nb.value]], tip_reads=is_tip[:nr].tolist())
    if steps & 1:
        res["out_tip_count"] = number(text, "Number of out-tip edges:", last=False)
        res["tip_count"] = number(text, "Final number of tip edges:", last=False)
    if steps & 2:
        res["transitive_kept"] = number(text, r"(?m)^(?=\d+ edges kept)")
        res["n_out_branch"] = number(text, "Number of nodes out-disconnected:")
        res["n_in_branch"] = number(text, "Number of nodes in-disconnected:")
        res["n_components"] = number(text, "Total number of components")
        res["n_removed_branches"] = number(text, "Number of edges removed:")
        res["n_tied_lists"] = int(stats[1])
        assert None not in (res["transitive_kept"], res["n_out_branch"], res["n_in_branch"], res["n_components"], res["n_removed_branches"]), text
    return res, ext[:2 * n].reshape(-1, 2), (float(stats[2]), float(stats[3]))


# ---- inputs ------------------------------------------------------------------------------------------------------------

def E(v1, v2, pos1=10, len1=90, pos2=0, len2=0, ori=(1, 1), od="-", r1=None, r2=None):
    return [v1, v2, v1 if r1 is None else r1, v2 if r2 is None else r2, pos1, pos2, len1, len2, ori[0], ori[1], ord(od)]


def singles(V, length=100):
    return [[length, 0, 0] for _ in range(V)]


def interval_case(seed, n, reach, n_tips, length=100):
    """Single-end reads of `length` bases tiled along a genome, read i -> read j when j starts less than `reach` after i
    (pos1 = the distance, the overlap = length - pos1), the out-lists shuffled; then short reads that dangle off both ends
    of random reads: a read that extends its neighbour by a few bases (or by none: contained) and points nowhere, and one
    that nothing points at."""
    rng = random.Random(seed)
    pos = sorted(rng.sample(range(n * 12), n))
    edges = []
    for i in range(n):
        lst = [E(i, j, pos1=pos[j] - pos[i], len1=length - (pos[j] - pos[i])) for j in range(i + 1, n) if pos[j] - pos[i] < reach]
        rng.shuffle(lst)
        edges += lst
    reads = singles(n, length)
    V = n
    for _ in range(n_tips):
        i = rng.randrange(2, n - 2)
        short = rng.choice([30, 45, 60])
        ext = rng.choice([0, 0, 3, 8, 20])       # bases by which the dangling read sticks out
        if rng.random() < 0.5:                   # i -> t, t a dead end
            edges.append(E(i, V, pos1=length - short + ext, len1=short - ext if ext else short))
        else:                                    # t -> i, nothing enters t
            edges.append(E(V, i, pos1=ext, len1=short - ext if ext else short))
        reads.append([short, 0, 0])
        V += 1
    rng.shuffle(edges)
    return V, edges, reads


def alltips_case():
    """Vertices all of whose out-edges (in-edges) end in dead ends: without an inclusion tip nothing goes; with one, only it."""
    e = []
    e += [E(0, 1, len1=95), E(0, 2, len1=92), E(0, 3, len1=97)]                 # out, all tips, none with ext_len 0
    e += [E(4, 5, len1=95), E(4, 6, len1=100), E(4, 7, len1=97)]                # out, all tips, 4 -> 6 an inclusion tip
    e += [E(8, 11, pos1=4), E(9, 11, pos1=7), E(10, 11, pos1=2)]                # in, all tips
    e += [E(12, 15, pos1=4), E(13, 15, pos1=0), E(14, 15, pos1=2)]              # in, all tips, 13 -> 15 an inclusion tip
    e += [E(16, 17, len1=95), E(16, 18, len1=60), E(18, 19, len1=60)]           # out, one tip beside an edge that leads on
    e += [E(20, 23, pos1=3), E(21, 23, pos1=40), E(22, 21, pos1=40)]            # in, likewise
    return 24, e, singles(24)


def alltips_only_case():
    return 8, [E(0, 1, len1=95), E(0, 2, len1=92), E(0, 3, len1=97), E(4, 7, pos1=4), E(5, 7, pos1=7), E(6, 7, pos1=2)], singles(8)


def both_passes_case():
    """0 -> 1 is a tip of the out-pass (1 is a dead end, 0 -> 2 leads on) and of the in-pass (nothing enters 0, 3 -> 1 comes from
    a vertex that has an in-edge): found twice, removed once."""
    e = [E(0, 1, pos1=5, len1=95), E(0, 2, pos1=40, len1=60), E(2, 5, pos1=40, len1=60), E(3, 1, pos1=40, len1=60), E(4, 3, pos1=40, len1=60)]
    return 6, e, singles(6)


def repeated_case(seed):
    """Repeated pairs (the two orientation classes of one pair): a list of at most 16 and one of more than 16 entries,
    whose targets are dead ends or lead on."""
    rng = random.Random(seed)
    V = 90
    edges = []
    for i in range(40, 80):                       # a backbone the lists point into
        edges.append(E(i, i + 1, pos1=50, len1=50))
    for (u, deg) in ((0, 7), (1, 24), (2, 40)):
        for t in rng.sample(range(3, 85), deg):
            edges.append(E(u, t, pos1=rng.choice([0, 3, 60]), len1=rng.choice([100, 97, 40]), ori=(1, 1)))
            if rng.random() < 0.6:
                edges.append(E(u, t, pos1=rng.choice([0, 3, 60]), len1=rng.choice([100, 97, 40]), ori=(1, 0)))
            if rng.random() < 0.2:
                edges.append(E(t, u, pos1=rng.choice([0, 3, 60]), len1=rng.choice([100, 97, 40]), ori=(0, 1)))
    rng.shuffle(edges)
    return V, edges, singles(V)


def hubs_case(seed):
    rng = random.Random(seed)
    V, edges, reads = interval_case(seed, 120, 30, 10)
    for j in range(V):
        if j not in (7, 11) and rng.random() < 0.9:
            edges.append(E(7, j, pos1=rng.choice([2, 30, 70]), len1=rng.choice([98, 70, 30])))
        if j not in (7, 11) and rng.random() < 0.9:
            edges.append(E(j, 11, pos1=rng.choice([2, 30, 70]), len1=rng.choice([98, 70, 30])))
    rng.shuffle(edges)
    return V, edges, reads


def duplicates_case(seed):
    """--add_duplicates: vertices [0, n) and their reverse complements [n, 2n) over n reads; every edge once more between the copies."""
    n, edges, reads = interval_case(seed, 40, 35, 12)
    out = list(edges)
    for e in edges:
        m = list(e)
        m[0], m[1] = e[1] + n, e[0] + n
        m[2], m[3] = e[3], e[2]
        m[8], m[9] = 1 - e[9], 1 - e[8]
        out.append(m)
    random.Random(seed).shuffle(out)
    return 2 * n, out, reads


def typed_case(seed):
    """All four read-type combinations with ord 1 / 2 / -, both ori2, lengths on both sides of every max(.., 0), negative
    pos1 + pos2.  Vertices below 50 have out-edges, vertices from 25 on have in-edges: plenty of dead ends on both sides."""
    rng = random.Random(seed)
    V = 90
    reads = []
    for _ in range(V):
        p = rng.random() < 0.5
        reads.append([rng.choice([60, 100, 140]), rng.choice([50, 100, 150]) if p else 0, 1 if p else 0])
    edges = []
    for _ in range(420):
        a, b = rng.randrange(50), rng.randrange(25, V)
        if a == b:
            continue
        edges.append(E(a, b, pos1=rng.choice([-9, -2, 0, 0, 4, 30, 90]), pos2=rng.choice([-7, 0, 0, 3, 25, 80]), len1=rng.choice([40, 60, 100, 140]),
                       len2=rng.choice([0, 30, 50, 100, 150]), ori=(rng.randrange(2), rng.randrange(2)), od=rng.choice("12-")))
    return V, edges, reads


def cycle_case():
    """A directed cycle, a chain, a chain with a branch, isolated vertices."""
    e = [E(i, (i + 1) % 7, pos1=50, len1=50) for i in range(7)]
    e += [E(i, i + 1, pos1=50, len1=50) for i in range(10, 16)]
    e += [E(i, i + 1, pos1=50, len1=50) for i in range(20, 26)] + [E(22, 27, pos1=50, len1=50), E(27, 28, pos1=50, len1=50),
                                                                    E(20, 22, pos1=80, len1=20)]
    random.Random(3).shuffle(e)
    return 32, e, singles(32)


def cases():
    V, e, r = interval_case(1, 70, 30, 24)
    for mt in (0, 150, 1):
        yield f"interval_mt{mt}", V, e, r, mt
    yield "alltips", *alltips_case(), 150
    yield "alltips_only", *alltips_only_case(), 150
    yield "both_passes", *both_passes_case(), 150
    yield "repeated", *repeated_case(5), 150
    yield "hubs", *hubs_case(6), 150
    yield "duplicates", *duplicates_case(7), 150
    V, e, r = typed_case(8)
    for mt in (0, 150, 40):
        yield f"typed_mt{mt}", V, e, r, mt
    yield "cycle", *cycle_case(), 150
    yield "isolated", 30, [x for x in interval_case(9, 30, 35, 0)[1] if x[0] % 5 and x[1] % 5], singles(30), 150
    yield "empty", 4, [], singles(4), 150


def ext_branch(e, reads, forward):
    """Which branch of Edge::ext_len (src/Edge.h:220-275) the edge takes, from its inputs."""
    t1, t2, od, ori2 = reads[e[2]][2], reads[e[3]][2], chr(e[10]), e[9]
    if not forward:
        return "b:pos1" if t1 and t2 and od == "1" else "b:pos1+pos2"
    if (t1 and t2 and od == "1") or (not t1 and not t2):
        return "f:PP1" if t1 else "f:SS"
    if t1 and t2 and od == "2":
        return f"f:PP2/ori2={ori2}"
    if not t1 and t2:
        return f"f:SP/ori2={ori2}"
    return "f:PS" if not t2 else "f:PP-"


ALL_BRANCHES = {"b:pos1", "b:pos1+pos2", "f:PP1", "f:SS", "f:PP2/ori2=0", "f:PP2/ori2=1", "f:SP/ori2=0", "f:SP/ori2=1", "f:PS", "f:PP-"}


def evaluated_branches(V, edges, reads):
    """The ext_len branches removeTips evaluates on the graph as given (out-pass: a source of more than one out-edge and a
    dead-end target; in-pass likewise on adj_in, on the first record of the pair)."""
    outdeg, indeg = [0] * V, [0] * V
    for e in edges:
        outdeg[e[0]] += 1
        indeg[e[1]] += 1
    hit, first = set(), {}
    for e in edges:
        first.setdefault((e[0], e[1]), e)
    for e in edges:
        if outdeg[e[0]] > 1 and outdeg[e[1]] == 0:
            hit.add(ext_branch(e, reads, True))
        if indeg[e[1]] > 1 and indeg[e[0]] == 0:
            hit.add(ext_branch(first[(e[0], e[1])], reads, False))
    return hit


def cycle_vertices(V, edges, var):
    """Vertices of the result that lie on a directed cycle all of whose vertices have one out- and one in-edge."""
    nxt, indeg = {}, [0] * V
    deg = np.diff(np.array(var["out_off"], np.int64))
    k = 0
    for v in range(V):
        for _ in range(int(deg[v])):
            w = edges[var["out"][k]][1]
            indeg[w] += 1
            if deg[v] == 1:
                nxt[v] = w
            k += 1
    on = set()
    for v in list(nxt):
        seen, x = [], v
        while x in nxt and indeg[x] == 1 and x not in seen:
            seen.append(x)
            x = nxt[x]
        if x == v and seen:
            on.update(seen)
    return on


def main():
    out_cases, hit = [], set()
    cond = dict(removed_lt_tips=False, alltips_nothing_removed=False, cycle_component=False, tied=False, negative_sum=False)
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        for name, V, edges, reads, mt in cases():
            variants = {}
            for vname, steps in VARIANTS:
                res, ext, _ = run(dll, V, edges, reads, mt, steps)
                variants[vname] = res
            hit |= evaluated_branches(V, edges, reads)
            t = variants["tips"]
            n_removed = len(t["branching"])
            cond["removed_lt_tips"] |= 0 < n_removed < t["tip_count"]
            cond["alltips_nothing_removed"] |= t["tip_count"] > 0 and n_removed == 0
            b = variants["branches"]
            cond["cycle_component"] |= b["n_components"] > 1 and len(cycle_vertices(V, edges, b)) > 0
            cond["tied"] |= b["n_tied_lists"] > 0
            cond["negative_sum"] |= any(e[4] + e[5] < 0 for e in edges) and t["tip_count"] > 0
            print(f"{name}: V={V} edges={len(edges)} max_tip_len={mt} tips={t['tip_count']} removed={n_removed} "
                  f"components={b['n_components']} branch-removed={len(b['branching'])} tied={b['n_tied_lists']}")
            out_cases.append(dict(name=name, V=V, max_tip_len=mt, edges_in=edges, reads=reads, variants=variants))
        timing = None
        if len(sys.argv) > 1:
            V, edges, reads = interval_case(11, 20000, 640, 2000, length=1000)
            _, _, (t_tips, _) = run(dll, V, edges, reads, 150, 1)
            _, _, (_, t_br) = run(dll, V, edges, reads, 150, 2)
            timing = dict(V=V, edges=len(edges), remove_tips_seconds=t_tips, remove_branches_seconds=t_br)
            print("timing", timing)
    assert hit == ALL_BRANCHES, sorted(ALL_BRANCHES - hit)
    assert all(cond.values()), cond
    doc = dict(note="OverlapGraph::removeTips + removeBranches of the reference (GraphAlgos.cpp:543-637, 714-743, 746-833, 835-936) through a "
                    "probe; edges_in = addEdge order, one record per entry: " + ",".join(FIELDS) + "; the full record of input k: score 1.0, "
                    "mismatch_rate 0.0, perc 100, pos3 = -3, pos4 = k, len0 = len1 + len2.  reads: len1,len2,paired per read.  "
                    "out / branching: input indices in list / removal order.",
               cases=out_cases)
    path = os.path.join(ROOT, "tests", "golden", "tips_branches.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
    if timing:
        with open(sys.argv[1], "w") as f:
            json.dump(timing, f)


if __name__ == "__main__":
    main()
