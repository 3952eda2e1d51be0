#!/usr/bin/env python3
"""Generates tests/golden/labelling.json with the reference's own OverlapGraph::vertexLabellingHeuristic and checkDuplicateEdges.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory: build-owned
declaration-only shells (below) around src/GraphAlgos.cpp:150-349 (sortVerticesByIndegree, vertexLabellingHeuristic, labelVertices) and
src/OverlapGraph.cpp:94-101 (addEdge), :150-194 (removeEdgeWithOri), :262-282 (getEdgeInfo), :578-605 (checkDuplicateEdges), streamed from
the reference by line range and never stored, with the genuine Types.h, Read.h and Edge.h.  A std::vector<bool> stands for the bitsets
(resize(n, true), indexing and assignment are all that is used).  The reference's addEdge and removeEdgeWithOri are compiled under
other names and called through shells that log the call, so the applied moves and deletions come back in the reference's order: a
removal followed by an addEdge is a move (the added Edge is the best try's copy), a removal alone a deletion.  The probe is built with
NDEBUG: checkDuplicateEdges' assert becomes its printed lines, from which the first place is read.  The number of tries is read from
the verbose output (a perfect labelling names it; otherwise the loop ran to 100).  Every input record carries its index as perc.

Also recorded: the permutations std::srand(s); std::random_shuffle applies, seeds 1..100, lengths 2..70 and 200: per seed the SHA-256 of
its permutations as bytes, back to back in length order, and seed 1's bytes themselves (base64).
The vectors are data; no reference source is stored.

With an argument: also times the reference's method on a 20 000-vertex graph and writes the seconds to that file.
"""
import base64
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

SHELL_HEAD = r"""
#include <assert.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <iostream>
#include <list>
#include <memory>
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
struct FastqStorage {
    unsigned int readcount;
    unsigned int get_readcount() { return readcount; }
};
struct Event { int kind; Edge edge; node_id_t v, w; bool opp; };

class OverlapGraph {
public:
    unsigned int vertex_count = 0;
    unsigned int edge_count = 0;
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    std::shared_ptr<FastqStorage> fastq_storage;
    ProgramSettings program_settings;
    boost::dynamic_bitset<> vertex_orientations;
    std::vector<Event> events;
    void addEdge(Edge edge) { events.push_back(Event{0, edge, 0, 0, false}); ref_addEdge(edge); }
    Edge removeEdgeWithOri(node_id_t v, node_id_t w, bool opposite_orientations) {
        Edge e = ref_removeEdgeWithOri(v, w, opposite_orientations);
        events.push_back(Event{1, e, v, w, opposite_orientations});
        return e;
    }
    void ref_addEdge(Edge edge);
    Edge ref_removeEdgeWithOri(node_id_t v, node_id_t w, bool opposite_orientations);
    Edge* getEdgeInfo(node_id_t v, node_id_t w, bool reverse_allowed = true);
    void checkDuplicateEdges();
    std::vector< node_id_t > sortVerticesByIndegree();
    void vertexLabellingHeuristic(unsigned int & conflict_count);
    void labelVertices(std::list< Edge > & edges_to_be_moved, std::list< Edge > & edges_to_be_deleted, boost::dynamic_bitset<> & orientations, int rand_seed);
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

// flags: 1 add_duplicates, 2 resolve_orientations.  ev: per event kind (0 added, 1 removed) and the Edge.  stats: edge_count,
// conflict_count, seconds.
extern "C" int label_probe(const frag_edge* in, uint64_t n, uint32_t V, uint32_t n_reads, uint32_t readcount, uint32_t flags, frag_edge* out,
                           uint64_t* out_off, uint64_t* in_off, uint64_t* in_nodes, uint8_t* orient, frag_edge* ev, uint8_t* ev_kind, uint64_t* n_ev,
                           uint64_t ev_cap, char* log, uint64_t log_cap, double* stats) {
    std::vector<Read> reads;
    reads.reserve(n_reads);
    for (uint32_t r = 0; r < n_reads; r++) reads.push_back(Read(false, false, r, std::string(10, 'A'), std::string(), std::string(10, 'I'), std::string()));
    OverlapGraph g;
    g.program_settings = ProgramSettings();
    g.program_settings.verbose = true;
    g.program_settings.add_duplicates = (flags & 1) != 0;
    g.program_settings.resolve_orientations = (flags & 2) != 0;
    g.fastq_storage = std::make_shared<FastqStorage>();
    g.fastq_storage->readcount = readcount;
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
        g.ref_addEdge(e);
    }
    std::ostringstream captured;
    std::streambuf* old = std::cout.rdbuf(captured.rdbuf());
    unsigned int conflict_count = 0;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    g.vertexLabellingHeuristic(conflict_count);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    g.checkDuplicateEdges();
    std::cout.rdbuf(old);
    const std::string text = captured.str();
    if (log_cap) {
        const size_t k = std::min<size_t>(text.size(), log_cap - 1);
        memcpy(log, text.c_str(), k);
        log[k] = 0;
    }
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
    for (uint32_t v = 0; v < V; v++) orient[v] = g.vertex_orientations[v] ? 1 : 0;
    *n_ev = g.events.size();
    for (size_t i = 0; i < g.events.size() && i < ev_cap; i++) ev[i] = flat(g.events[i].edge, base), ev_kind[i] = (uint8_t)g.events[i].kind;
    stats[0] = g.edge_count;
    stats[1] = conflict_count;
    stats[2] = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    return 0;
}

extern "C" void shuffle_probe(unsigned int seed, uint32_t n, uint32_t* perm) {
    std::vector<uint32_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = i;
    std::srand(seed);
    std::random_shuffle(v.begin(), v.end());
    for (uint32_t i = 0; i < n; i++) perm[i] = v[i];
}
"""

# the reference's addEdge / removeEdgeWithOri get the shells' names for them
RANGES = [("GraphAlgos.cpp", 150, 349, ()), ("OverlapGraph.cpp", 94, 101, (("OverlapGraph::addEdge", "OverlapGraph::ref_addEdge"),)),
          ("OverlapGraph.cpp", 150, 194, (("OverlapGraph::removeEdgeWithOri", "OverlapGraph::ref_removeEdgeWithOri"),)),
          ("OverlapGraph.cpp", 262, 282, ()), ("OverlapGraph.cpp", 578, 605, ())]

FIELDS = ["v1", "v2", "read1", "read2", "pos1", "pos2", "pos3", "pos4", "ori1", "ori2", "ord", "perc"]
EDGE_FIELDS = ["v1", "v2", "ori1", "ori2", "pos1", "pos2", "pos3", "pos4", "ord"]  # an input record


class FragEdge(C.Structure):
    _fields_ = [("score", C.c_double), ("mismatch_rate", C.c_double), ("pos1", C.c_int32), ("pos2", C.c_int32), ("pos3", C.c_int32),
                ("pos4", C.c_int32), ("ori1", C.c_uint8), ("ori2", C.c_uint8), ("ord", C.c_uint8), ("pad", C.c_uint8), ("read1", C.c_uint32),
                ("read2", C.c_uint32), ("pad2", C.c_uint32), ("v1", C.c_uint64), ("v2", C.c_uint64), ("perc", C.c_int32), ("len0", C.c_int32),
                ("len1", C.c_int32), ("len2", C.c_int32)]


def build_probe(tmp, flags=("-O2",)):
    src = [SHELL_HEAD]
    for f, a, b, renames in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        for old, new in renames:
            src.append(f"#define {old.split('::')[1]} {new.split('::')[1]}\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n")
        for old, _ in renames:
            src.append(f"#undef {old.split('::')[1]}\n")
    src.append(SHELL_TAIL)
    lib = os.path.join(tmp, "liblabelprobe.so")
    subprocess.run(["g++", *flags, "-DNDEBUG", "-Wno-deprecated-declarations", "-std=c++14", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib],
                   input="".join(src), text=True, check=True)
    dll = C.CDLL(lib)
    dll.label_probe.restype = C.c_int
    dll.label_probe.argtypes = [C.c_void_p, C.c_uint64] + [C.c_uint32] * 4 + [C.c_void_p] * 8 + [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    dll.shuffle_probe.restype = None
    dll.shuffle_probe.argtypes = [C.c_uint, C.c_uint32, C.c_void_p]
    return dll


def to_struct(e, k):
    return FragEdge(1.0, 0.25, e["pos1"], e["pos2"], e["pos3"], e["pos4"], e["ori1"], e["ori2"], ord(e["ord"]), 0, e["v1"], e["v2"], 0, e["v1"], e["v2"],
                    k, 30, 20, 10)


def flat(o):
    return [int(getattr(o, f)) for f in FIELDS]


def run(dll, V, edges, flags, readcount, want_log=True):
    n = len(edges)
    arr = (FragEdge * max(n, 1))()
    for k, e in enumerate(edges):
        arr[k] = to_struct(e, k)
    out, ev = (FragEdge * max(n, 1))(), (FragEdge * max(3 * n, 1))()
    ev_kind = np.zeros(max(3 * n, 1), np.uint8)
    out_off, in_off = np.zeros(V + 1, np.uint64), np.zeros(V + 1, np.uint64)
    in_nodes, orient = np.zeros(max(n, 1), np.uint64), np.zeros(max(V, 1), np.uint8)
    n_ev = C.c_uint64()
    log = C.create_string_buffer(1 << 16)
    stats = np.zeros(3, np.float64)
    rc = dll.label_probe(arr, n, V, V, readcount, flags, out, out_off.ctypes.data, in_off.ctypes.data, in_nodes.ctypes.data, orient.ctypes.data, ev,
                         ev_kind.ctypes.data, C.byref(n_ev), 3 * n, log, len(log), stats.ctypes.data)
    assert rc == 0, rc
    text = log.value.decode()
    m = int(out_off[V])
    moved, deleted, k = [], [], 0
    while k < n_ev.value:  # a removal followed by an addEdge is a move
        assert ev_kind[k] == 1
        if k + 1 < n_ev.value and ev_kind[k + 1] == 0:
            moved.append(flat(ev[k + 1]))
            k += 2
        else:
            deleted.append([int(ev[k].v1), int(ev[k].v2), int(ev[k].ori1 == ev[k].ori2), int(ev[k].perc)])
            k += 1
    perfect = re.search(r"perfect labelling was found after (\d+) tries", text)
    tries = 0 if not (flags & 2) or (flags & 1) else int(perfect.group(1)) if perfect else 100
    dup = re.search(r"(\d+) to (\d+) duplicate", text)
    status, bad_v, bad_pos = 0, 0, 0
    if dup:
        status, bad_v = 1, int(dup.group(1))
        tg = [int(o.v2) for o in out[int(out_off[bad_v]):int(out_off[bad_v + 1])]]
        bad_pos = next(p for p in range(1, len(tg)) if tg[p] == tg[p - 1])
    return dict(edge_count=int(stats[0]), conflict_count=int(stats[1]), tries=tries, out=[flat(o) for o in out[:m]], out_off=out_off.tolist(),
                in_off=in_off.tolist(), in_nodes=in_nodes[:m].tolist(), orientations=orient[:V].tolist(), moved=moved, deleted=deleted, status=status,
                bad_v=bad_v, bad_pos=bad_pos, seconds=float(stats[2]))


def edge(v1, v2, o1=1, o2=1, pos1=5, pos2=0, pos3=7, pos4=0, od="-"):
    return dict(v1=v1, v2=v2, ori1=o1, ori2=o2, pos1=pos1, pos2=pos2, pos3=pos3, pos4=pos4, ord=od)


def hidden_label_graph(rng, V, n_edges, n_odd=0, first=0, paired=True):
    """Random simple digraph on [first, first + V) whose classes follow a hidden labelling, n_odd records against it; positions and ord
    drawn so that every branch of switch_edge_orientation is met."""
    h = [rng.randrange(2) for _ in range(V)]
    seen, es = set(), []
    for v in range(1, V):  # a spanning tree first: one component
        u = rng.randrange(v)
        a, b = (u, v) if rng.random() < 0.5 else (v, u)
        seen.add((a, b)), seen.add((b, a))
        es.append((a, b))
    while len(es) < n_edges:
        a, b = rng.randrange(V), rng.randrange(V)
        if a == b or (a, b) in seen:
            continue
        seen.add((a, b)), seen.add((b, a))
        es.append((a, b))
    rng.shuffle(es)
    odd = set(rng.sample(range(len(es)), n_odd))
    out = []
    for k, (a, b) in enumerate(es):
        o1, o2 = h[a], h[b]
        if rng.random() < 0.5:
            o1, o2 = 1 - o1, 1 - o2
        if k in odd:
            o2 = 1 - o2
        od = rng.choice("-12") if paired else "-"
        out.append(edge(first + a, first + b, o1, o2, pos1=rng.randrange(0, 9), pos2=rng.randrange(0, 9) if od != "-" else 0, pos3=rng.choice((-3, -1, 0, 0, 0, 2, 4)),
                        pos4=rng.randrange(-4, 5) if od != "-" else 0, od=od))
    return out


def hub_lists(first=0):
    """Three hubs with 63 / 64 / 65 out-records over shared targets, classes from a hidden labelling."""
    rng = random.Random(77)
    V = 3 + 65
    h = [rng.randrange(2) for _ in range(V)]
    out = []
    for hub, deg in ((0, 63), (1, 64), (2, 65)):
        for t in range(deg):
            v = 3 + t
            o1, o2 = h[hub], h[v]
            if rng.random() < 0.5:
                o1, o2 = 1 - o1, 1 - o2
            out.append(edge(first + hub, first + v, o1, o2, pos1=rng.randrange(0, 9), pos3=rng.randrange(-4, 5)))
    return V, out


def cases():
    rng = random.Random(20240521)
    R, A = 2, 1
    cs = []
    cs.append(("all_plus_plus", 6, [edge(0, 1), edge(1, 2), edge(0, 2), edge(3, 4)], R, 0))
    cs.append(("isolated_only", 4, [], R, 0))
    cs.append(("consistent_forced", 30, hidden_label_graph(rng, 24, 60), R, 0))  # vertices 24..29 isolated
    cs.append(("two_chains_id_tie", 8, [edge(4, 5, 0, 0, pos3=2), edge(5, 6, 0, 1, pos3=-2), edge(0, 1, 1, 0, pos3=0), edge(1, 2, 0, 0, pos3=3)], R, 0))
    cs.append(("triangle_one_odd", 3, [edge(0, 1), edge(1, 2), edge(0, 2, 1, 0)], R, 0))
    cs.append(("odd_next_to_consistent", 9, [edge(0, 1), edge(1, 2), edge(2, 0, 1, 0)] + hidden_label_graph(rng, 6, 9, first=3), R, 0))
    for k, (V, E, n_odd) in enumerate(((12, 30, 2), (16, 40, 3), (20, 60, 5), (9, 20, 1))):
        cs.append((f"inconsistent_{k}", V, hidden_label_graph(rng, V, E, n_odd), R, 0))
    # vertex 3 has two shortest paths from the start vertex 0, of different parity: which one labels it depends on the try's shuffle of
    # 0's neighbours, so 3 -> 4 is switched in place back and forth, and one of 3 -> 5 / 3 -> 6 is moved at the best try
    cs.append(("flip_flop", 7, [edge(0, 1), edge(0, 2), edge(1, 3), edge(2, 3, 1, 0), edge(3, 4, 1, 1, pos2=1, pos3=3, pos4=-2, od="2"),
                                edge(3, 5, 1, 1, pos3=-1), edge(3, 6, 0, 0, pos3=-1)], R, 0))
    cs.append(("pair_both_classes", 5, [edge(0, 1), edge(1, 0, 1, 0, pos3=3), edge(1, 2), edge(2, 3, 0, 0, pos3=-1), edge(3, 4)], R, 0))
    cs.append(("pair_both_classes_same_direction", 4, [edge(0, 1), edge(0, 1, 0, 1, pos3=2), edge(1, 2, 0, 0), edge(2, 3)], R, 0))
    V, hub = hub_lists()
    cs.append(("lists_63_64_65", V, hub, R, 0))
    g = hidden_label_graph(rng, 10, 18)
    cs.append(("add_duplicates", 10, g, A, 5))
    cs.append(("resolve_off", 10, g, 0, 0))
    cs.append(("duplicate_edge_fires", 5, [edge(0, 1), edge(0, 2), edge(0, 2, 1, 0), edge(3, 4), edge(3, 4, 0, 1)], 0, 0))
    return cs


def check_coverage(golden):
    by = {c["name"]: c for c in golden}

    def same_record(c, o):
        return [c["edges"][o[11]][f] if f != "ord" else ord(c["edges"][o[11]][f]) for f in ("v1", "v2", "ori1", "ori2", "pos1", "pos3", "ord")] == \
            [o[0], o[1], o[8], o[9], o[4], o[6], o[10]]

    c = by["all_plus_plus"]
    assert all(same_record(c, o) for o in c["out"]) and not c["moved"] and c["tries"] == 1 and all(c["orientations"])
    c = by["consistent_forced"]
    assert c["tries"] == 1 and c["conflict_count"] == 0
    inplace = [o for o in c["out"] if o[0] == c["edges"][o[11]]["v1"] and o[8] != c["edges"][o[11]]["ori1"]]
    assert inplace, "no record switched in place"
    assert any(c["edges"][m[11]]["pos3"] < 0 for m in c["moved"]), "no move by pos1 < 0"
    assert any(c["edges"][m[11]]["pos3"] == 0 and c["edges"][m[11]]["v1"] > c["edges"][m[11]]["v2"] for m in c["moved"]), "no move by pos1 == 0"
    touched = inplace + c["moved"]
    for before, after in (("-", "-"), ("1", "2"), ("2", "1"), ("1", "1"), ("2", "2")):
        assert any(c["edges"][o[11]]["ord"] == before and chr(o[10]) == after for o in touched), f"no ord outcome {before} -> {after}"
    assert any(c["out_off"][v] == c["out_off"][v + 1] and c["in_off"][v] == c["in_off"][v + 1] for v in range(c["V"])), "no isolated vertex"
    c = by["two_chains_id_tie"]
    assert c["orientations"][0] == 1 and c["orientations"][4] == 1 and c["in_off"][1] == c["in_off"][0] and c["in_off"][5] == c["in_off"][4]
    assert by["triangle_one_odd"]["tries"] == 100 and by["triangle_one_odd"]["conflict_count"] >= 1
    c = by["odd_next_to_consistent"]
    assert c["tries"] == 100 and c["conflict_count"] >= 1 and (c["moved"] or any(not same_record(c, o) for o in c["out"] if o[0] >= 3))
    # switched in place more than once: the orientations are the input's again but the record is not (pos4 < 0 came back negated)
    c = by["flip_flop"]
    def once(e):  # a record switched in place exactly once (the branch of switch_edge_orientation that keeps the direction)
        pos2, od = (-e["pos4"], "2") if e["pos4"] < 0 else (e["pos4"], e["ord"] if e["ord"] == "-" else "1")
        return [e["pos3"], pos2, e["pos1"], e["pos2"], 1 - e["ori1"], 1 - e["ori2"], ord(od)]

    def as_is(e):
        return [e["pos1"], e["pos2"], e["pos3"], e["pos4"], e["ori1"], e["ori2"], ord(e["ord"])]

    twice = [o for o in c["out"] if o[0] == c["edges"][o[11]]["v1"] and o[4:11] not in (as_is(c["edges"][o[11]]), once(c["edges"][o[11]]))]
    assert twice, "no record switched in place in one try and again in a later one"
    assert c["tries"] == 100 and len(c["moved"]) == 1, "no record moved at the best try while later tries go on"
    assert any(by[f"inconsistent_{k}"]["moved"] for k in range(4))
    assert by["pair_both_classes"]["tries"] == 100 and by["pair_both_classes_same_direction"]["tries"] == 100
    c = by["lists_63_64_65"]
    assert [c["out_off"][v + 1] - c["out_off"][v] for v in range(3)] != [0, 0, 0] and len(c["edges"]) == 63 + 64 + 65
    c = by["add_duplicates"]
    assert c["orientations"] == [1] * 5 + [0] * 5 and all(same_record(c, o) for o in c["out"]) and c["tries"] == 0
    c = by["resolve_off"]
    assert all(c["orientations"]) and all(same_record(c, o) for o in c["out"])
    c = by["duplicate_edge_fires"]
    assert (c["status"], c["bad_v"], c["bad_pos"]) == (1, 0, 2)


def timing(dll, path):
    rng = random.Random(5)
    V = 20000
    es = hidden_label_graph(rng, V, 10 * V, paired=False)
    t0 = time.time()
    res = run(dll, V, es, 2, 0)
    with open(path, "w") as f:
        json.dump(dict(V=V, E=len(es), seconds_method=res["seconds"], seconds_with_build=time.time() - t0, moved=len(res["moved"]), tries=res["tries"]), f)
        f.write("\n")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        golden = []
        for name, V, edges, flags, readcount in cases():
            res = run(dll, V, edges, flags, readcount)
            res.pop("seconds")
            golden.append(dict(name=name, V=V, flags=flags, n_reads=readcount, edges=edges, **res))
        check_coverage(golden)
        for c in golden:  # (the input records as rows: the file stays small)
            c["edges"] = [[e[f] for f in EDGE_FIELDS] for e in c["edges"]]
        lengths = list(range(2, 71)) + [200]
        digests, first = [], b""
        buf = np.zeros(256, np.uint32)
        for seed in range(1, 101):
            blob = bytearray()
            for n in lengths:
                dll.shuffle_probe(seed, n, buf.ctypes.data)
                blob += bytes(buf[:n].astype(np.uint8))
            digests.append(hashlib.sha256(bytes(blob)).hexdigest())
            first = first or bytes(blob)
        out = dict(fields=FIELDS, edge_fields=EDGE_FIELDS, cases=golden,
                   shuffles=dict(seeds=[1, 100], lengths=lengths, sha256_by_seed=digests, seed1_b64=base64.b64encode(first).decode()))
        path = os.path.join(ROOT, "tests", "golden", "labelling.json")
        with open(path, "w") as f:
            json.dump(out, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {path}: {len(golden)} cases, {os.path.getsize(path)} bytes")
        if len(sys.argv) > 1:
            timing(dll, sys.argv[1])


if __name__ == "__main__":
    main()
