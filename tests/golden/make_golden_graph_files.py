#!/usr/bin/env python3
"""Generates tests/golden/graph_files.json with the reference's own OverlapGraph::writeGraphToFile, writeDiGraphToFile and
write2GFA.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory:
build-owned declaration-only shells (below) around src/OverlapGraph.cpp:94-102 (addEdge), :233-259 (checkEdge), :322-385
(writeGraphToFile), :388-409 (writeDiGraphToFile) and :468-543 (write2GFA), streamed from the reference by line range and
never stored, with the genuine Types.h, Read.h, Edge.h and FastqStorage.h.  A std::vector<bool> stands for the `inclusions`
bitset, which is only indexed on the path taken (`verbose` is false while writeGraphToFile runs, so the .count() of :339
is never called; the stand-in gives it a one-line body so that the probe loads).  The probe builds each graph by addEdge
calls in the order given over reads built from the read table, writes the three files into the temporary directory
(writeGraphToFile's own `cat` runs there) and hands back L_count / C_count, which write2GFA prints when `verbose` is on.
The script reads the files back and stores them with the inputs.  The vectors are data; no reference source is stored.

With an argument: also times the three functions on a 200 000-vertex interval graph of 150-base single-end reads and
writes the seconds to that file (not stored in the golden file).
"""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

SHELL_HEAD = r"""
#include <assert.h>
#include <stdint.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "Types.h"
#include "Read.h"
#include "Edge.h"
#include "FastqStorage.h"

void FastqStorage::read_singles() {}
void FastqStorage::read_pairs() {}
void FastqStorage::read_new_ids() {}

struct inclusion_bits : std::vector<bool> {
    size_t count() const { return (size_t)std::count(begin(), end(), true); }
};

class OverlapGraph {
public:
    unsigned int vertex_count = 0;
    unsigned int edge_count = 0;
    std::string PATH;
    std::shared_ptr<FastqStorage> fastq_storage;
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    inclusion_bits inclusions;
    ProgramSettings program_settings;
    void addEdge(Edge edge);
    double checkEdge(node_id_t v, node_id_t w, bool reverse_allowed);
    void writeGraphToFile();
    void writeDiGraphToFile();
    void write2GFA(std::string filename);
};
"""

SHELL_TAIL = r"""
struct frag_edge {
    double score, mismatch_rate;
    int32_t pos1, pos2, len1, len2, perc;
    uint32_t read1, read2, v1, v2;
    uint8_t ori1, ori2, ord, pad;
};
struct frag_read { const char* seq1; const char* seq2; uint32_t paired; uint32_t pad; };

static double seconds(const timespec& a, const timespec& b) { return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec); }

// out[0], out[1]: L_count, C_count; out[2..4]: seconds of the three functions
extern "C" int graph_files_probe(const char* dir, const frag_edge* in, uint64_t n, uint32_t V, const uint8_t* incl, const frag_read* rd,
                                 uint32_t n_reads, uint32_t n_singles, double edge_threshold, double merge_contigs, double* out) {
    std::vector<Read> reads;
    reads.reserve(n_reads);
    for (uint32_t r = 0; r < n_reads; r++) {
        const std::string s1(rd[r].seq1), s2(rd[r].seq2);
        reads.push_back(Read(rd[r].paired != 0, false, r, s1, s2, std::string(s1.size(), 'I'), std::string(s2.size(), 'I')));
    }
    ProgramSettings ps = ProgramSettings();
    ps.output_dir = dir;
    ps.edge_threshold = edge_threshold;
    ps.merge_contigs = merge_contigs;
    ps.verbose = false;
    OverlapGraph g;
    g.program_settings = ps;
    g.PATH = dir;
    g.fastq_storage = std::make_shared<FastqStorage>(ps);
    for (uint32_t r = 0; r < n_reads; r++) g.fastq_storage->m_read_vec.push_back(&reads[r]);
    g.fastq_storage->m_readcount_single = n_singles;
    g.vertex_count = V;
    g.adj_out.assign(V, std::list<Edge>());
    g.adj_in.assign(V, std::list<node_id_t>());
    g.inclusions.assign(V, false);
    for (uint32_t v = 0; v < V; v++) g.inclusions[v] = incl[v] != 0;
    for (uint64_t i = 0; i < n; i++) {
        const frag_edge& r = in[i];
        if (r.v1 >= V || r.v2 >= V || r.read1 >= n_reads || r.read2 >= n_reads) return 1;
        Edge e(r.score, r.pos1, r.pos2, r.ori1 != 0, r.ori2 != 0, std::string(1, (char)r.ord), &reads[r.read1], &reads[r.read2]);
        e.set_vertices(r.v1, r.v2);
        e.set_perc(r.perc);
        e.set_len(r.len1, r.len2);
        e.set_mismatch(r.mismatch_rate);
        g.addEdge(e);
    }
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    g.writeGraphToFile();
    clock_gettime(CLOCK_MONOTONIC, &t1);
    out[2] = seconds(t0, t1);
    clock_gettime(CLOCK_MONOTONIC, &t0);
    g.writeDiGraphToFile();
    clock_gettime(CLOCK_MONOTONIC, &t1);
    out[3] = seconds(t0, t1);
    g.program_settings.verbose = true;
    std::ostringstream captured;
    std::streambuf* old = std::cout.rdbuf(captured.rdbuf());
    clock_gettime(CLOCK_MONOTONIC, &t0);
    g.write2GFA(g.PATH + "graph.gfa");
    clock_gettime(CLOCK_MONOTONIC, &t1);
    std::cout.rdbuf(old);
    out[4] = seconds(t0, t1);
    const std::string text = captured.str();
    unsigned long lc = 0, cc = 0;
    const size_t a = text.find("L_count = "), b = text.find("C_count = ");
    if (a == std::string::npos || b == std::string::npos) return 2;
    lc = strtoul(text.c_str() + a + 10, NULL, 10);
    cc = strtoul(text.c_str() + b + 10, NULL, 10);
    out[0] = (double)lc;
    out[1] = (double)cc;
    return 0;
}
"""

RANGES = [("OverlapGraph.cpp", 94, 102), ("OverlapGraph.cpp", 233, 259), ("OverlapGraph.cpp", 322, 385), ("OverlapGraph.cpp", 388, 409),
          ("OverlapGraph.cpp", 468, 543)]


class FragEdge(C.Structure):
    _fields_ = [("score", C.c_double), ("mismatch_rate", C.c_double), ("pos1", C.c_int32), ("pos2", C.c_int32), ("len1", C.c_int32),
                ("len2", C.c_int32), ("perc", C.c_int32), ("read1", C.c_uint32), ("read2", C.c_uint32), ("v1", C.c_uint32), ("v2", C.c_uint32),
                ("ori1", C.c_uint8), ("ori2", C.c_uint8), ("ord", C.c_uint8), ("pad", C.c_uint8)]


class FragRead(C.Structure):
    _fields_ = [("seq1", C.c_char_p), ("seq2", C.c_char_p), ("paired", C.c_uint32), ("pad", C.c_uint32)]


def build_probe(tmp, flags=("-O2",)):
    src = [SHELL_HEAD]
    for f, a, b in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n")
    src.append(SHELL_TAIL)
    lib = os.path.join(tmp, "libgraphfilesprobe.so")
    subprocess.run(["g++", *flags, "-std=c++14", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib], input="".join(src), text=True,
                   check=True)
    dll = C.CDLL(lib)
    dll.graph_files_probe.restype = C.c_int
    dll.graph_files_probe.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double,
                                      C.c_double, C.POINTER(C.c_double)]
    return dll


# one record per edge, the first eleven as in tips_branches.json
FIELDS = ["v1", "v2", "read1", "read2", "pos1", "pos2", "len1", "len2", "ori1", "ori2", "ord", "score", "mismatch_rate", "perc"]


def run(dll, tmp, case):
    V, edges, reads = case["V"], case["edges_in"], case["reads"]
    n, nr = len(edges), len(reads)
    arr = (FragEdge * max(n, 1))()
    for k, (v1, v2, r1, r2, p1, p2, l1, l2, o1, o2, od, sc, mm, pc) in enumerate(edges):
        arr[k] = FragEdge(sc, mm, p1, p2, l1, l2, pc, r1, r2, v1, v2, o1, o2, od, 0)
    rd = (FragRead * max(nr, 1))()
    for k, (s1, s2, p) in enumerate(reads):
        rd[k] = FragRead(s1.encode(), s2.encode(), p, 0)
    out = (C.c_double * 5)()
    d = os.path.join(tmp, "case") + "/"
    os.makedirs(d, exist_ok=True)
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    rc = dll.graph_files_probe(d.encode(), arr, n, V, bytes(case["inclusions"]), rd, nr, case["n_singles"], case["edge_threshold"],
                               case["merge_contigs"], out)
    assert rc == 0, rc
    assert sorted(os.listdir(d)) == ["digraph.txt", "graph.gfa", "graph.txt"], os.listdir(d)
    files = {f: open(os.path.join(d, f), "rb").read().decode("ascii") for f in os.listdir(d)}
    return files, int(out[0]), int(out[1]), (out[2], out[3], out[4])


# ---- inputs ------------------------------------------------------------------------------------------------------------

def E(v1, v2, score=0.99, mm=0.0, perc=60, len1=40, len2=0, pos1=10, pos2=0, ori=(1, 1), od="-", n_reads=None):
    r1, r2 = (v1, v2) if n_reads is None else (v1 % n_reads, v2 % n_reads)
    return [v1, v2, r1, r2, pos1, pos2, len1, len2, ori[0], ori[1], ord(od), score, mm, perc]


def seqs(rng, lengths, paired_from=None, alphabet="ACGTN"):
    """One read per length; reads from index paired_from on are pairs (a second sequence of another length)."""
    out = []
    for k, n in enumerate(lengths):
        p = paired_from is not None and k >= paired_from
        s1 = "".join(rng.choice(alphabet) for _ in range(n))
        s2 = "".join(rng.choice(alphabet) for _ in range(n + 3)) if p else ""
        out.append([s1, s2, 1 if p else 0])
    return out


def case(name, V, edges, reads, n_singles, inclusions=None, edge_threshold=0.9, merge_contigs=0.0):
    return dict(name=name, V=V, n_singles=n_singles, edge_threshold=edge_threshold, merge_contigs=merge_contigs,
                inclusions=list(inclusions) if inclusions is not None else [0] * V, reads=reads, edges_in=edges)


def random_case(name, seed, n_reads, n_singles, duplicates, n_edges, n_incl):
    """A random graph without self-loops: shuffled lists, repeated pairs, reverse pairs with scores on both sides of 0, inclusion
    vertices without out-edges; every record passes checkEdge's assert (score >= edge_threshold or mismatch_rate <= merge_contigs)."""
    rng = random.Random(seed)
    V = 2 * n_reads if duplicates else n_reads
    incl = [0] * V
    for v in rng.sample(range(V), n_incl):
        incl[v] = 1
    sources = [v for v in range(V) if not incl[v]]
    edges = []
    while len(edges) < n_edges:
        a, b = rng.choice(sources), rng.randrange(V)
        if a == b:
            continue
        score = rng.choice([0.99, 0.95, 0.5, 0.0, -1.0, 1e-300])
        mm = 0.0 if score < 0.9 else rng.choice([0.0, 0.02, 0.3])
        e = E(a, b, score=score, mm=mm, perc=rng.choice([100, 100, 99, 60, 0]), len1=rng.choice([1, 9, 40, 150]), len2=rng.choice([0, 0, 35]),
              pos1=rng.choice([0, 7, 110]), ori=(rng.randrange(2), rng.randrange(2)), od=rng.choice("12-"), n_reads=n_reads)
        edges.append(e)
        if rng.random() < 0.35 and not incl[b]:  # the reverse record, sometimes twice
            for _ in range(rng.choice([1, 1, 2])):
                s2 = rng.choice([0.99, 0.0, -1.0, 0.5])
                edges.append(E(b, a, score=s2, mm=0.0 if s2 < 0.9 else 0.1, perc=rng.choice([100, 80]), n_reads=n_reads))
        if rng.random() < 0.15:
            edges.append(E(a, b, score=rng.choice([0.99, 0.0]), perc=rng.choice([100, 30]), len1=77, n_reads=n_reads))
    rng.shuffle(edges)
    lengths = [rng.choice([1, 2, 15, 16, 17, 31, 40, 64, 65]) for _ in range(n_reads)]
    return case(name, V, edges, seqs(rng, lengths, paired_from=n_singles), n_singles, incl, edge_threshold=0.9, merge_contigs=0.05)


def cases():
    rng = random.Random(1)
    r6 = seqs(rng, [12, 20, 16, 9, 33, 17])
    # reverse pairs: seen from the larger vertex (j < i: checkEdge decides) and from the smaller one (j > i: always written)
    yield case("reverse_pair", 6, [E(3, 1), E(1, 3), E(0, 4), E(4, 0), E(5, 2)], r6, 6)
    yield case("reverse_pair_zero_score", 6, [E(3, 1), E(1, 3, score=0.0), E(4, 0), E(0, 4, score=-1.0), E(5, 2), E(2, 5, score=1e-300)], r6, 6,
               edge_threshold=-2.0)
    yield case("repeated", 6, [E(0, 2), E(0, 2, perc=100), E(0, 2, len1=7), E(4, 1), E(4, 1), E(1, 4), E(1, 4)], r6, 6)
    # j -> i twice: the first copy's score decides
    yield case("first_copy_zero", 6, [E(1, 3, score=0.0), E(1, 3, score=0.99), E(3, 1)], r6, 6, edge_threshold=0.0)
    yield case("first_copy_positive", 6, [E(1, 3, score=0.99), E(1, 3, score=0.0), E(3, 1)], r6, 6, edge_threshold=0.0)
    yield case("first_copy_behind_others", 6, [E(1, 0), E(1, 5), E(1, 3, score=-1.0), E(1, 4), E(1, 3, score=0.99), E(3, 1), E(3, 1)], r6, 6,
               edge_threshold=-1.0)
    # an inclusion vertex with an empty list; records whose target is one
    yield case("inclusion_vertex", 6, [E(0, 2), E(1, 2), E(3, 2), E(3, 4), E(4, 3), E(5, 2), E(5, 0), E(0, 5)], r6, 6, inclusions=[0, 0, 1, 0, 0, 0])
    yield case("inclusion_all_targets", 4, [E(0, 3), E(1, 3), E(2, 3)], r6[:4], 4, inclusions=[0, 0, 0, 1])
    # paired reads between the singles and the end: their vertices and edges are skipped in GFA
    rp = seqs(rng, [14, 16, 18, 20, 22, 24], paired_from=3)
    yield case("paired_reads", 6, [E(0, 1), E(0, 4), E(4, 0), E(3, 5), E(1, 2, perc=100), E(2, 5), E(5, 1), E(2, 0)], rp, 3)
    yield case("no_singles", 6, [E(0, 1), E(2, 3)], seqs(rng, [10] * 6, paired_from=0), 0)
    # --add_duplicates: V = 2 * n_reads, vertices [n, 2n) are the reverse complements
    rd = seqs(rng, [1, 15, 16, 17, 40])
    yield case("duplicates", 10, [E(0, 1, n_reads=5), E(6, 5, n_reads=5), E(2, 8, n_reads=5), E(7, 3, n_reads=5), E(9, 0, perc=100, n_reads=5),
                                  E(4, 9, n_reads=5), E(5, 6, score=0.0, n_reads=5)], rd, 5, edge_threshold=0.0)
    rdp = seqs(rng, [13, 16, 19, 21], paired_from=2)
    yield case("duplicates_paired", 8, [E(0, 1, n_reads=4), E(5, 4, n_reads=4), E(1, 6, n_reads=4), E(2, 0, n_reads=4), E(4, 7, n_reads=4),
                                        E(7, 3, n_reads=4), E(4, 1, perc=100, n_reads=4)], rdp, 2)
    # perc of 100 and below
    yield case("perc", 6, [E(0, 1, perc=100), E(0, 2, perc=99), E(1, 2, perc=0), E(2, 3, perc=100), E(4, 5, perc=100, len1=150, len2=150)], r6, 6)
    # ids across 9 / 10 and 99 / 100
    r110 = seqs(rng, [rng.choice([3, 8, 16, 21]) for _ in range(110)])
    yield case("digit_boundaries", 110, [E(9, 10), E(10, 9), E(9, 8), E(99, 100), E(100, 99), E(100, 9), E(10, 100), E(109, 0), E(0, 109, score=0.0),
                                         E(99, 98), E(98, 99)], r110, 110, edge_threshold=0.0)
    yield case("digit_boundaries_duplicates", 110, [E(9, 10, n_reads=55), E(54, 55, n_reads=55), E(55, 54, n_reads=55), E(99, 100, n_reads=55),
                                                    E(100, 64, n_reads=55), E(64, 9, n_reads=55)], r110[:55], 55)
    yield case("edgeless", 5, [], r6[:5], 5)
    yield case("edgeless_inclusions", 4, [], r6[:4], 2, inclusions=[1, 0, 1, 1])
    yield case("one_vertex", 1, [], r6[:1], 1)
    yield random_case("random_singles", 11, 24, 24, False, 90, 3)
    yield random_case("random_mixed", 12, 24, 15, False, 90, 2)
    yield random_case("random_duplicates", 13, 14, 14, True, 100, 3)
    yield random_case("random_duplicates_mixed", 14, 14, 9, True, 100, 2)
    yield random_case("random_dense", 15, 8, 8, False, 120, 0)
    yield random_case("random_sparse", 16, 36, 30, False, 25, 6)


def interval_case(n, reach, length=150, seed=5):
    rng = random.Random(seed)
    pos = sorted(rng.sample(range(n * 12), n))
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            d = pos[j] - pos[i]
            if d >= reach:
                break
            edges.append(E(i, j, pos1=d, len1=length - d if d < length else 1, perc=100 if d == 0 else 60))
    return case("timing", n, edges, seqs(rng, [length] * n, alphabet="ACGT"), n)


def main():
    out_cases = []
    seen = dict(skipped_reverse=False, written_reverse=False, repeated=False, incl_target=False, paired=False, reverse_range=False,
                contained=False, link=False)
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        for c in cases():
            files, lc, cc, _ = run(dll, tmp, c)
            g = files["graph.txt"].split("\n")
            assert int(g[0]) == c["V"] and int(g[1]) == len(g) - 3, c["name"]
            n_seg = len(re.findall(r"(?m)^S\t", files["graph.gfa"]))
            assert lc + cc == len(re.findall(r"(?m)^L\t", files["graph.gfa"])), c["name"]
            c["expected"] = dict(graph_txt=files["graph.txt"], digraph_txt=files["digraph.txt"], gfa=files["graph.gfa"], n_pairs=int(g[1]) // 2,
                                 n_segments=n_seg, l_count=lc, c_count=cc)
            pairs = [(e[0], e[1]) for e in c["edges_in"]]
            written = set(tuple(map(int, x.split(","))) for x in g[2:-1])
            for (a, b) in pairs:
                if a > b and (b, a) in pairs and not c["inclusions"][a] and not c["inclusions"][b]:
                    seen["skipped_reverse" if int(g[1]) // 2 < len(pairs) else "written_reverse"] = True
            seen["written_reverse"] |= c["name"] in ("reverse_pair_zero_score", "first_copy_zero") and int(g[1]) // 2 == len(pairs)
            seen["repeated"] |= len(set(pairs)) < len(pairs) and len(written) < int(g[1])
            seen["incl_target"] |= any(c["inclusions"][b] for _, b in pairs)
            seen["paired"] |= any(r[2] for r in c["reads"]) and n_seg > 0
            seen["reverse_range"] |= c["V"] == 2 * len(c["reads"]) and n_seg > c["n_singles"]
            seen["contained"] |= cc > 0
            seen["link"] |= lc > 0
            print(f"{c['name']}: V={c['V']} edges={len(pairs)} pairs={int(g[1]) // 2} segments={n_seg} L={lc} C={cc}")
            out_cases.append(c)
        timing = None
        if len(sys.argv) > 1:
            c = interval_case(200000, 240)
            _, _, _, (t_g, t_d, t_f) = run(dll, tmp, c)
            timing = dict(V=c["V"], edges=len(c["edges_in"]), write_graph_seconds=t_g, write_digraph_seconds=t_d, write_gfa_seconds=t_f)
            print("timing", timing)
    assert all(seen.values()), seen
    doc = dict(note="OverlapGraph::writeGraphToFile, writeDiGraphToFile and write2GFA of the reference (OverlapGraph.cpp:322-385, 388-409, "
                    "468-543) through a probe; edges_in = addEdge order, one record per entry: " + ",".join(FIELDS) + " (len0 = len1 + len2, "
                    "pos3 = pos4 = 0).  reads: seq1,seq2,paired per read, the first n_singles of them single-end; V = the reads or twice the "
                    "reads (--add_duplicates).  expected: the three files and the counts (L_count / C_count as write2GFA prints them).",
               cases=out_cases)
    path = os.path.join(ROOT, "tests", "golden", "graph_files.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
    if timing:
        with open(sys.argv[1], "w") as f:
            json.dump(timing, f)


if __name__ == "__main__":
    main()
