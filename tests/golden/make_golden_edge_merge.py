#!/usr/bin/env python3
"""Generates tests/golden/edge_merge.json with the reference's own SRBuilder::sort_vertices, SRBuilder::calcSubreadInfo,
OverlapGraph::getEdgeInfo and OverlapGraph::getEdgesForMerging.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory:
build-owned declaration-only shells (below) around src/SRBuilder.cpp:33-285 (sort_vertices, whose closing brace the probe adds), :536-595 (calcSubreadInfo),
:654-698 (the head of constructSuperread: the sort of the clique, the type / base choice and the sort_vertices calls; the
probe closes the function behind line 698 with an ending of its own that hands the locals back), src/OverlapGraph.cpp:83-86
(getOrientation), :94-100 (addEdge, whose closing brace the probe adds), :263-282 (getEdgeInfo) and src/GraphAlgos.cpp:112-148 (getEdgesForMerging), streamed
from the reference by line range and never stored, with the genuine Types.h, Read.h, Edge.h and FastqStorage.h.  A
std::vector<bool> stands for the dynamic_bitset, which is only indexed; FastqStorage's file readers are empty and its get_read
indexes the read vector (read id = read index).

Every mate of every read is a distinct random string, so the probe's seq_list / qual_list entries are resolved here to
(read, mate, reverse-complemented) and checked against the quality strings.  calcSubreadInfo is run for several trim
positions per pair (its inputs besides the lists; -1 for trim_pos2 is what a failed consensus of the /2 layout returns).
The vectors are data; no reference source is stored.
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
PROVENANCE = ("SRBuilder::sort_vertices (SRBuilder.cpp:33-285), calcSubreadInfo (:536-595) and the head of constructSuperread (:654-698, "
              "genuine: it compiled in the shells with a build-owned ending) with OverlapGraph::getOrientation, addEdge, getEdgeInfo "
              "(OverlapGraph.cpp:83-86, 94-100, 263-282) and getEdgesForMerging (GraphAlgos.cpp:112-148) of the reference through a probe")

SHELL_HEAD = r"""
#include <assert.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "Types.h"
#include "Read.h"
#include "Edge.h"
#include "FastqStorage.h"
using std::bind2nd;

namespace boost {
template <class Block = unsigned long>
struct dynamic_bitset : std::vector<bool> {
    dynamic_bitset() {}
    explicit dynamic_bitset(size_t n) : std::vector<bool>(n, false) {}
};
}

void FastqStorage::read_singles() {}
void FastqStorage::read_pairs() {}
void FastqStorage::read_new_ids() {}
Read* FastqStorage::get_read(read_id_t ID) { return m_read_vec[m_ID_to_index.at(ID)]; }

class OverlapGraph {
public:
    unsigned int vertex_count = 0;
    unsigned int edge_count = 0;
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    std::vector<read_id_t> vertex_to_read;
    boost::dynamic_bitset<> vertex_orientations;
    bool getOrientation(node_id_t v);
    void addEdge(Edge edge);
    Edge* getEdgeInfo(node_id_t v, node_id_t w, bool reverse_allowed=true);
    std::vector< std::vector< node_id_t > > getEdgesForMerging();
};

struct ProbeOut {
    char type;
    node_id_t base;
    int len1, len2;
    std::list<int> pos1, pos2;
    std::list<std::string> seq1, seq2, qual1, qual2;
    std::list<node_id_t> sv1, sv2;
};
static ProbeOut g_out;

class SRBuilder {
public:
    FastqStorage* fastq_storage;
    OverlapGraph* overlap_graph;
    int sort_vertices(std::vector< node_id_t > vertices, char type, node_id_t base_node, std::list<int> &pos_list, std::list<std::string> &seq_list, std::list<std::string> &qual_list, std::list<node_id_t> &sorted_vertices, int thread_id);
    Read constructSuperread(std::vector<node_id_t> clique, read_id_t id, int thread_id);
    std::unordered_map< node_id_t, SubreadInfo > calcSubreadInfo(int trim_pos1, int trim_pos2, std::list<int> pos_list1, std::list<int> pos_list2, std::list<node_id_t> sorted_vertices1, std::list<node_id_t> sorted_vertices2);
};
"""

# closes constructSuperread behind src/SRBuilder.cpp:698
ENDING = r"""
    g_out.type = superread_type;
    g_out.base = base_node;
    g_out.len1 = len1;
    g_out.len2 = len2;
    g_out.pos1 = pos_list1; g_out.pos2 = pos_list2;
    g_out.seq1 = seq_list1; g_out.seq2 = seq_list2;
    g_out.qual1 = qual_list1; g_out.qual2 = qual_list2;
    g_out.sv1 = sorted_vertices1; g_out.sv2 = sorted_vertices2;
    (void)id;
    return *fastq_storage->get_read(0);
}
"""

SHELL_TAIL = r"""
struct frag_edge { int32_t pos1, pos2; uint32_t read1, read2, v1, v2; uint8_t ori1, ori2, ord, pad; };
struct frag_read { uint64_t off1, off2; uint32_t len1, len2; uint8_t paired, pad[7]; };

static OverlapGraph* g_graph = nullptr;
static FastqStorage* g_fastq = nullptr;
static std::vector<Read>* g_reads = nullptr;

extern "C" int em_setup(const frag_edge* in, uint64_t n, uint32_t V, const frag_read* rd, uint32_t n_reads, const char* bases, const char* quals,
                        const uint32_t* vertex_read, const uint8_t* vertex_fwd) {
    delete g_graph; delete g_fastq; delete g_reads;
    ProgramSettings ps = ProgramSettings();
    ps.output_dir = ""; ps.singles_file = ""; ps.paired1_file = ""; ps.paired2_file = ""; ps.id_correspondence = ""; ps.verbose = false;
    g_fastq = new FastqStorage(ps);
    g_reads = new std::vector<Read>();
    g_reads->reserve(n_reads);
    for (uint32_t r = 0; r < n_reads; r++) {
        g_reads->push_back(Read(rd[r].paired != 0, false, r, std::string(bases + rd[r].off1, rd[r].len1), std::string(bases + rd[r].off2, rd[r].len2),
                                std::string(quals + rd[r].off1, rd[r].len1), std::string(quals + rd[r].off2, rd[r].len2)));
    }
    for (uint32_t r = 0; r < n_reads; r++) {
        g_fastq->m_read_vec.push_back(&(*g_reads)[r]);
        g_fastq->m_ID_to_index.insert(std::make_pair((read_id_t)r, (unsigned int)r));
    }
    g_graph = new OverlapGraph();
    g_graph->vertex_count = V;
    g_graph->adj_out.assign(V, std::list<Edge>());
    g_graph->adj_in.assign(V, std::list<node_id_t>());
    g_graph->vertex_orientations = boost::dynamic_bitset<>(V);
    for (uint32_t v = 0; v < V; v++) {
        g_graph->vertex_to_read.push_back(vertex_read[v]);
        g_graph->vertex_orientations[v] = vertex_fwd[v] != 0;
    }
    for (uint64_t i = 0; i < n; i++) {
        const frag_edge& r = in[i];
        if (r.v1 >= V || r.v2 >= V || r.read1 >= n_reads || r.read2 >= n_reads) return 1;
        Edge e(1.0, r.pos1, r.pos2, r.ori1 != 0, r.ori2 != 0, std::string(1, (char)r.ord), &(*g_reads)[r.read1], &(*g_reads)[r.read2]);
        e.set_vertices(r.v1, r.v2);
        e.set_perc(100);
        g_graph->addEdge(e);
    }
    return 0;
}

extern "C" int64_t em_merge_pairs(uint32_t* out, uint64_t cap) {
    std::vector< std::vector< node_id_t > > v = g_graph->getEdgesForMerging();
    if (v.size() > cap) return -1;
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].size() != 2) return -2;
        out[2 * i] = (uint32_t)v[i][0];
        out[2 * i + 1] = (uint32_t)v[i][1];
    }
    return (int64_t)v.size();
}

static void put(std::ostringstream& o, const std::list<int>& pos, const std::list<std::string>& seq, const std::list<std::string>& qual,
                const std::list<node_id_t>& sv) {
    o << pos.size() << "\n";
    auto s = seq.begin(); auto q = qual.begin(); auto v = sv.begin();
    for (int p : pos) { o << p << " " << *v << " " << *s << " " << *q << "\n"; ++s; ++q; ++v; }
}

// constructSuperread's head for the clique {v, w} as given; the lists as text
extern "C" int em_pair(uint32_t v, uint32_t w, char* text, uint64_t cap) {
    SRBuilder b;
    b.fastq_storage = g_fastq;
    b.overlap_graph = g_graph;
    std::vector<node_id_t> clique = {v, w};
    b.constructSuperread(clique, 0, 0);
    std::ostringstream o;
    o << g_out.type << " " << g_out.base << " " << g_out.len1 << " " << g_out.len2 << "\n";
    put(o, g_out.pos1, g_out.seq1, g_out.qual1, g_out.sv1);
    put(o, g_out.pos2, g_out.seq2, g_out.qual2, g_out.sv2);
    const std::string t = o.str();
    if (t.size() + 1 > cap) return 1;
    memcpy(text, t.c_str(), t.size() + 1);
    return 0;
}

// calcSubreadInfo on the lists of the last em_pair; out: index1, startpos1, index2, startpos2 of vertex a, then of vertex b
extern "C" int em_subreads(int trim_pos1, int trim_pos2, uint32_t a, uint32_t b, int32_t* out) {
    SRBuilder s;
    s.fastq_storage = g_fastq;
    s.overlap_graph = g_graph;
    std::unordered_map< node_id_t, SubreadInfo > m = s.calcSubreadInfo(trim_pos1, trim_pos2, g_out.pos1, g_out.pos2, g_out.sv1, g_out.sv2);
    if (m.size() != 2 || !m.count(a) || !m.count(b)) return 1;
    const SubreadInfo x = m[a], y = m[b];
    out[0] = x.index1; out[1] = x.startpos1; out[2] = x.index2; out[3] = x.startpos2;
    out[4] = y.index1; out[5] = y.startpos1; out[6] = y.index2; out[7] = y.startpos2;
    return 0;
}
"""

# (file, first line, last line, build-owned text behind it)
RANGES = [("OverlapGraph.cpp", 83, 86, ""), ("OverlapGraph.cpp", 94, 100, "}\n"), ("OverlapGraph.cpp", 263, 282, ""), ("GraphAlgos.cpp", 112, 148, ""),
          ("SRBuilder.cpp", 33, 285, "}\n"), ("SRBuilder.cpp", 536, 595, ""), ("SRBuilder.cpp", 654, 698, ENDING)]


class FragEdge(C.Structure):
    _fields_ = [("pos1", C.c_int32), ("pos2", C.c_int32), ("read1", C.c_uint32), ("read2", C.c_uint32), ("v1", C.c_uint32), ("v2", C.c_uint32),
                ("ori1", C.c_uint8), ("ori2", C.c_uint8), ("ord", C.c_uint8), ("pad", C.c_uint8)]


class FragRead(C.Structure):
    _fields_ = [("off1", C.c_uint64), ("off2", C.c_uint64), ("len1", C.c_uint32), ("len2", C.c_uint32), ("paired", C.c_uint8), ("pad", C.c_uint8 * 7)]


def build_probe(tmp):
    src = [SHELL_HEAD]
    for f, a, b, behind in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n" + behind)
    src.append(SHELL_TAIL)
    lib = os.path.join(tmp, "libedgemergeprobe.so")
    subprocess.run(["g++", "-O1", "-std=c++14", "-w", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib], input="".join(src), text=True,
                   check=True)
    dll = C.CDLL(lib)
    dll.em_setup.restype = C.c_int
    dll.em_setup.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    dll.em_merge_pairs.restype = C.c_int64
    dll.em_merge_pairs.argtypes = [C.c_void_p, C.c_uint64]
    dll.em_pair.restype = C.c_int
    dll.em_pair.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64]
    dll.em_subreads.restype = C.c_int
    dll.em_subreads.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    return dll


COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
FIELDS = ["v1", "v2", "read1", "read2", "pos1", "pos2", "ori1", "ori2", "ord"]


def run_case(dll, V, edges, reads, vertex_read, vertex_fwd, pairs, rng):
    """edges: FIELDS rows in addEdge order; reads: [len1, len2, paired]; returns (merge pairs, per-pair results)."""
    n, nr = len(edges), len(reads)
    arr = (FragEdge * max(n, 1))()
    for k, (v1, v2, r1, r2, p1, p2, o1, o2, od) in enumerate(edges):
        arr[k] = FragEdge(p1, p2, r1, r2, v1, v2, o1, o2, od, 0)
    rd = (FragRead * max(nr, 1))()
    bases, quals, at, lookup = [], [], 0, {}
    for k, (l1, l2, p) in enumerate(reads):
        offs = []
        for mate, ln in ((1, l1), (2, l2)):
            s = "".join(rng.choice("ACGT") for _ in range(ln))
            q = "".join(chr(rng.randrange(35, 74)) for _ in range(ln))
            while ln and (s in lookup or "".join(COMP[c] for c in reversed(s)) in lookup):
                s = "".join(rng.choice("ACGT") for _ in range(ln))
            if ln:
                seq_no = mate if p else 0
                lookup[s] = (k, seq_no, 0, q)
                lookup["".join(COMP[c] for c in reversed(s))] = (k, seq_no, 1, q[::-1])
            bases.append(s)
            quals.append(q)
            offs.append(at)
            at += ln
        rd[k] = FragRead(offs[0], offs[1], l1, l2, p)
    vr = np.asarray(vertex_read, np.uint32)
    vf = np.asarray(vertex_fwd, np.uint8)
    assert dll.em_setup(arr, n, V, rd, nr, "".join(bases).encode(), "".join(quals).encode(), vr.ctypes.data, vf.ctypes.data) == 0
    mp = np.zeros((V + 1, 2), np.uint32)
    k = dll.em_merge_pairs(mp.ctypes.data, V + 1)
    assert k >= 0
    merge = mp[:k].tolist()
    text = C.create_string_buffer(1 << 14)
    out = []
    for (v, w) in pairs:
        assert dll.em_pair(v, w, text, len(text)) == 0
        lines = text.value.decode().split("\n")
        typ, base, len1, len2 = lines[0].split()
        at = 1
        lists = []
        for _ in range(2):
            cnt = int(lines[at])
            ent = []
            for ln in lines[at + 1:at + 1 + cnt]:
                pos, vertex, s, q = ln.split()
                read, seq_no, rev, want_q = lookup[s]
                assert q == want_q, "the quality string does not go with the sequence"
                ent.append([read, seq_no, rev, int(pos), int(vertex)])
            lists.append(ent)
            at += 1 + cnt
        a, b = min(v, w), max(v, w)
        positions = sorted({e[3] for e in lists[0] + lists[1]})
        last = positions[-1]
        trims = [(0, -1), (3, -1), (last, -1), (-1, -1), (last + 4, -1)] if typ == "s" else [(0, -1), (3, 0), (last, 2), (-1, last + 1), (2, 5)]
        subs = []
        buf = np.zeros(8, np.int32)
        for t1, t2 in trims:
            assert dll.em_subreads(t1, t2, a, b, buf.ctypes.data) == 0
            subs.append([t1, t2, buf[:4].tolist(), buf[4:].tolist()])
        out.append(dict(pair=[v, w], type=typ, base=int(base), total_len=[int(len1), int(len2)][:2 if typ == "p" else 1],
                        lists=lists[:2 if typ == "p" else 1], subreads=subs))
    return merge, out


# ---- inputs ------------------------------------------------------------------------------------------------------------

class Builder:
    def __init__(self):
        self.reads, self.vread, self.vfwd, self.edges, self.pairs = [], [], [], [], []

    def vertex(self, paired, fwd, l1, l2=0):
        self.reads.append([l1, l2 if paired else 0, 1 if paired else 0])
        self.vread.append(len(self.reads) - 1)
        self.vfwd.append(1 if fwd else 0)
        return len(self.vread) - 1

    def edge(self, v1, v2, pos1, pos2, od, swap_reads=False):
        r1, r2 = self.vread[v1], self.vread[v2]
        if swap_reads:
            r1, r2 = r2, r1
        self.edges.append([v1, v2, r1, r2, pos1, pos2, self.vfwd[v1], self.vfwd[v2], ord(od)])

    def case(self, name, pairs=None):
        return name, len(self.vread), self.edges, self.reads, self.vread, self.vfwd, self.pairs if pairs is None else pairs


def matrix_case():
    """All four type combinations x both orientations of each vertex x base as read 1 / read 2 x ord '1' / '2' / '-' x the record
    as base -> node or only as node -> base, with new_pos negative, 0 and positive."""
    b = Builder()
    rng = random.Random(21)
    for pa in (0, 1):
        for pb in (0, 1):
            for fa in (0, 1):
                for fb in (0, 1):
                    for swap in (False, True):
                        for od in "12-":
                            for direction in (0, 1):
                                for pos1 in (-7, 0, 12):
                                    va = b.vertex(pa, fa, rng.choice([40, 55, 70]), rng.choice([35, 50, 64]))
                                    vb = b.vertex(pb, fb, rng.choice([40, 55, 70]), rng.choice([35, 50, 64]))
                                    neg2 = pa and pb                 # a negative pos2 only where no mate 2 of an 's' layout takes it (:227)
                                    pos2 = rng.choice([-9, 0, 5, 30] if neg2 else [0, 5, 30])
                                    # base -> node or node -> base: the base is va unless only vb is single-end
                                    base, node = (vb, va) if (pa and not pb) else (va, vb)
                                    src, dst = (base, node) if direction == 0 else (node, base)
                                    b.edge(src, dst, pos1, pos2, od, swap)
                                    b.pairs.append([va, vb] if rng.random() < 0.5 else [vb, va])
    return b.case("matrix")


def special_case():
    b = Builder()
    # all three entries of an 's'-with-paired layout at one position: [mate 2, mate 1, base]
    s, p = b.vertex(0, 1, 50), b.vertex(1, 1, 60, 45)
    b.edge(s, p, 0, 0, "-")
    b.pairs.append([s, p])
    # the right extension decided by mate 1
    s, p = b.vertex(0, 1, 50), b.vertex(1, 0, 60, 60)
    b.edge(s, p, 30, 0, "1")
    b.pairs.append([p, s])
    # mate 1 left of the base, mate 2 right of it; and both left
    s, p = b.vertex(0, 0, 50), b.vertex(1, 1, 40, 70)
    b.edge(p, s, 11, 20, "2")
    b.pairs.append([s, p])
    p, s = b.vertex(1, 1, 40, 70), b.vertex(0, 1, 80)
    b.edge(p, s, 25, 0, "-")
    b.pairs.append([p, s])
    # a pair repeated in a list with different pos1: the first record wins; also present in the reverse list
    x, y, z = b.vertex(0, 1, 60), b.vertex(0, 1, 60), b.vertex(0, 1, 60)
    b.edge(x, z, 3, 0, "-")
    b.edge(x, y, 17, 0, "-")
    b.edge(x, y, 5, 0, "-")
    b.edge(y, x, 9, 0, "-")
    b.pairs += [[x, y], [y, x], [x, z]]
    # the edge present only as node -> base, behind other records
    x, y, z = b.vertex(1, 1, 60, 60), b.vertex(1, 0, 50, 66), b.vertex(1, 1, 44, 44)
    b.edge(y, z, 1, 2, "1")
    b.edge(y, x, 14, 22, "2")
    b.edge(y, x, 2, 3, "1")
    b.pairs += [[x, y], [y, z]]
    # paired base as read 2 with ord 1 and 2, negative results for 'r'
    for od in "12":
        x, y = b.vertex(1, 0, 52, 48), b.vertex(1, 1, 61, 39)
        b.edge(y, x, 8, 13, od)
        b.pairs.append([x, y])
    return b.case("special")


def chain_case(n=12):
    b = Builder()
    vs = [b.vertex(i % 3 == 0, i % 2, 50 + i, 40) for i in range(n)]
    for i in range(n - 1):
        b.edge(vs[i], vs[i + 1], 10 + i, 4, "1")
    return b.case("chain", "merge")


def star_case():
    b = Builder()
    vs = [b.vertex(0, 1, 60) for _ in range(8)]
    for i in (3, 1, 5, 7):
        b.edge(vs[0], vs[i], 5 + i, 0, "-")
    for i in (2, 4):
        b.edge(vs[i], vs[0], 6, 0, "-")
    b.edge(vs[2], vs[6], 9, 0, "-")
    return b.case("star", "merge")


def early_target_case():
    """2 is taken as 0's target before its own turn; 1 then passes over 2 and takes 3; 2's and 3's own lists are skipped; 4 finds
    every target marked."""
    b = Builder()
    vs = [b.vertex(i == 5, 1, 60, 50) for i in range(8)]
    b.edge(vs[0], vs[2], 4, 0, "-")
    b.edge(vs[0], vs[1], 5, 0, "-")
    b.edge(vs[1], vs[2], 6, 0, "-")
    b.edge(vs[1], vs[3], 7, 0, "-")
    b.edge(vs[2], vs[4], 8, 0, "-")
    b.edge(vs[3], vs[5], 9, 0, "-")
    b.edge(vs[4], vs[2], 3, 0, "-")
    b.edge(vs[4], vs[0], 2, 0, "-")
    b.edge(vs[6], vs[5], 11, 3, "-")
    b.edge(vs[6], vs[7], 12, 0, "-")
    return b.case("early_target", "merge")


def main():
    rng = random.Random(7)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        for name, V, edges, reads, vread, vfwd, pairs in (matrix_case(), special_case(), chain_case(), star_case(), early_target_case()):
            if pairs == "merge":  # lay out what getEdgesForMerging picks
                merge, _ = run_case(dll, V, edges, reads, vread, vfwd, [], rng)
                pairs = merge
            merge, out = run_case(dll, V, edges, reads, vread, vfwd, pairs, rng)
            print(f"{name}: V={V} edges={len(edges)} pairs={len(pairs)} merge_pairs={len(merge)}")
            cases.append(dict(name=name, V=V, edges_in=edges, reads=reads, vertex_read=vread, vertex_fwd=vfwd, merge_pairs=merge, pairs=out))
    # what the cases must include
    allp = [p for c in cases for p in c["pairs"]]
    pos = [e[3] for p in allp for l in p["lists"] for e in l]
    assert {p["type"] for p in allp} == {"s", "p"}
    assert any(len(l) == 3 and len({e[3] for e in l}) == 1 for p in allp for l in p["lists"]), "three entries at one position"
    assert min(pos) == 0 and max(pos) > 0
    assert any(len(p["lists"][0]) == 3 and p["lists"][0][0][4] != p["base"] and p["lists"][0][-1][4] != p["base"] for p in allp), "base in the middle"
    doc = dict(note=PROVENANCE + ".  edges_in = addEdge order, one record per entry: " + ",".join(FIELDS) + " (score 1.0).  reads: len1,len2,paired "
                    "per read.  merge_pairs: getEdgesForMerging in the order taken.  pairs[]: the clique as given, type, base vertex, total_len per "
                    "layout ('l', 'r' or 's'), lists per layout in list order: read, seq (0 | 1 | 2), rev, pos (shifted), vertex; subreads: "
                    "trim_pos1, trim_pos2, then index1,startpos1,index2,startpos2 of the smaller and of the larger vertex.",
               cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "edge_merge.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
