#!/usr/bin/env python3
"""Generates tests/golden/clique_merge.json with the reference's own SRBuilder::constructSuperread for cliques of any size.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory: the build-owned
declaration shells of make_golden_edge_merge.py (its OverlapGraph, FastqStorage and dynamic_bitset stand-ins, imported from there, nothing of
it changed; the bitset gains count(), which consensus calls) around src/SRBuilder.cpp:33-285 (sort_vertices, whose closing brace the probe
adds), :289-535 (phred_to_prob, consensus_pos, consensus), :536-595 (calcSubreadInfo), :597-651 (filter_subreads, sortVerticesByEndpos) and
:654-748 (constructSuperread up to and including the calcSubreadInfo call; the probe closes the function behind line 748 with an ending of its
own that hands the locals back), with src/OverlapGraph.cpp:83-86, 94-100, 263-282, streamed from the reference by line range and never
stored.  No substitute beyond the shells: sort_vertices, filter_subreads with its std::sort, consensus and calcSubreadInfo are genuine.

The filtered lists are locals of a block inside constructSuperread; the probe calls the genuine filter_subreads once more on the exported
full lists (the function is deterministic) to export them.  Every mate of every read is a distinct random string, so the probe's seq_list
entries are resolved here to (read, mate, reverse-complemented).  The vectors are data; no reference source is stored.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_edge_merge as EM  # noqa: E402

ROOT = EM.ROOT
REF = EM.REF
PROVENANCE = ("SRBuilder::constructSuperread (SRBuilder.cpp:654-748, genuine up to the calcSubreadInfo call, with a build-owned ending) over "
              "sort_vertices (:33-285), consensus (:289-535), calcSubreadInfo (:536-595), filter_subreads and sortVerticesByEndpos (:597-651) and "
              "OverlapGraph::getOrientation, addEdge, getEdgeInfo (OverlapGraph.cpp:83-86, 94-100, 263-282) of the reference through a probe "
              "with no substitute beyond the declaration shells")

BITSET = "explicit dynamic_bitset(size_t n) : std::vector<bool>(n, false) {}"
CLASS = r"""
#include <cmath>
struct CliqueOut {
    char type;
    node_id_t base;
    int len1, len2, trim1, trim2;
    size_t cons1, cons2;
    std::list<int> pos1, pos2;
    std::list<std::string> seq1, seq2, qual1, qual2;
    std::list<node_id_t> sv1, sv2;
    std::unordered_map< node_id_t, SubreadInfo > sub;
};
static CliqueOut g_c;

class SRBuilder {
public:
    FastqStorage* fastq_storage;
    OverlapGraph* overlap_graph;
    ProgramSettings program_settings;
    double minQual;
    int sort_vertices(std::vector< node_id_t > vertices, char type, node_id_t base_node, std::list<int> &pos_list, std::list<std::string> &seq_list, std::list<std::string> &qual_list, std::list<node_id_t> &sorted_vertices, int thread_id);
    double phred_to_prob(const int phred);
    bool consensus_pos(std::string nucleotides, std::string qualities, std::string &cons_seq, std::string& cons_qual);
    int consensus(int total_len, std::list<int> &pos_list, std::list<std::string> &seq_list, std::list<std::string> &qual_list, std::string &cons_seq, std::string &cons_qual, bool subreads_needed, bool error_correction);
    std::unordered_map< node_id_t, SubreadInfo > calcSubreadInfo(int trim_pos1, int trim_pos2, std::list<int> pos_list1, std::list<int> pos_list2, std::list<node_id_t> sorted_vertices1, std::list<node_id_t> sorted_vertices2);
    void filter_subreads(int num, node_id_t base_node, std::list< node_id_t > & sorted_vertices, std::list<int> & pos_list, std::list< std::string > & seq_list, std::list< std::string > & qual_list, std::list<int> & new_pos_list, std::list< std::string> & new_seq_list, std::list< std::string > & new_qual_list);
    std::vector< node_id_t > sortVerticesByEndpos(std::vector< std::pair<node_id_t, int> > pairs);
    Read constructSuperread(std::vector<node_id_t> clique, read_id_t id, int thread_id);
};
"""

# closes constructSuperread behind src/SRBuilder.cpp:748
ENDING = r"""
    g_c.type = superread_type;
    g_c.base = base_node;
    g_c.len1 = len1; g_c.len2 = len2;
    g_c.trim1 = trim_pos1; g_c.trim2 = trim_pos2;
    g_c.cons1 = cons_seq1.size(); g_c.cons2 = cons_seq2.size();
    g_c.pos1 = pos_list1; g_c.pos2 = pos_list2;
    g_c.seq1 = seq_list1; g_c.seq2 = seq_list2;
    g_c.qual1 = qual_list1; g_c.qual2 = qual_list2;
    g_c.sv1 = sorted_vertices1; g_c.sv2 = sorted_vertices2;
    g_c.sub = subreads_map;
    (void)id;
    return *fastq_storage->get_read(0);
}
"""

TAIL = r"""
static void put_filtered(std::ostringstream& o, SRBuilder& b, int num, std::list<node_id_t>& sv, std::list<int>& pos, std::list<std::string>& seq,
                         std::list<std::string>& qual) {
    std::list<int> np;
    std::list<std::string> ns, nq;
    b.filter_subreads(num, g_c.base, sv, pos, seq, qual, np, ns, nq);
    o << np.size() << "\n";
    auto s = ns.begin();
    for (int p : np) { o << p << " " << *s << "\n"; ++s; }
}

// constructSuperread for the clique as given; the lists, the filtered lists, the trim positions and the subread map as text
extern "C" int cm_clique(const uint32_t* nodes, uint32_t n, uint32_t min_clique_size, int error_correction, char* text, uint64_t cap) {
    SRBuilder b;
    b.fastq_storage = g_fastq;
    b.overlap_graph = g_graph;
    b.program_settings = ProgramSettings();
    b.program_settings.min_clique_size = min_clique_size;
    b.program_settings.error_correction = error_correction != 0;
    b.program_settings.first_it = true;
    b.program_settings.verbose = false;
    b.minQual = 0.99;
    std::vector<node_id_t> clique(nodes, nodes + n);
    b.constructSuperread(clique, 0, 0);
    std::ostringstream o;
    o << g_c.type << " " << g_c.base << " " << g_c.len1 << " " << g_c.len2 << " " << g_c.trim1 << " " << g_c.trim2 << " " << g_c.cons1 << " " << g_c.cons2 << "\n";
    put(o, g_c.pos1, g_c.seq1, g_c.qual1, g_c.sv1);
    put(o, g_c.pos2, g_c.seq2, g_c.qual2, g_c.sv2);
    if (n > 3 * min_clique_size) {
        put_filtered(o, b, 2 * min_clique_size, g_c.sv1, g_c.pos1, g_c.seq1, g_c.qual1);
        if (g_c.type == 'p') put_filtered(o, b, 2 * min_clique_size, g_c.sv2, g_c.pos2, g_c.seq2, g_c.qual2);
        else o << "0\n";
    } else {
        o << "-1\n-1\n";
    }
    std::vector<node_id_t> sorted(clique);
    std::sort(sorted.begin(), sorted.end());
    o << g_c.sub.size() << "\n";
    for (node_id_t v : sorted) {
        if (!g_c.sub.count(v)) return 2;
        const SubreadInfo x = g_c.sub[v];
        o << v << " " << x.index1 << " " << x.startpos1 << " " << x.index2 << " " << x.startpos2 << "\n";
    }
    const std::string t = o.str();
    if (t.size() + 1 > cap) return 1;
    memcpy(text, t.c_str(), t.size() + 1);
    return 0;
}
"""

# (file, first line, last line, build-owned text behind it)
RANGES = [("OverlapGraph.cpp", 83, 86, ""), ("OverlapGraph.cpp", 94, 100, "}\n"), ("OverlapGraph.cpp", 263, 282, ""), ("GraphAlgos.cpp", 112, 148, ""),
          ("SRBuilder.cpp", 33, 285, "}\n"), ("SRBuilder.cpp", 289, 535, ""), ("SRBuilder.cpp", 536, 595, ""), ("SRBuilder.cpp", 597, 651, ""),
          ("SRBuilder.cpp", 654, 748, ENDING)]


def build_probe(tmp):
    head = EM.SHELL_HEAD
    assert BITSET in head and "class SRBuilder {" in head
    head = head.replace(BITSET, BITSET + "\n    size_t count() const { size_t c = 0; for (bool b : *this) c += b; return c; }")
    head = head[:head.index("class SRBuilder {")] + CLASS
    src = [head]
    for f, a, b, behind in RANGES:
        with open(os.path.join(REF, f)) as fh:
            lines = fh.read().split("\n")
        src.append(f'#line {a} "{f}"\n' + "\n".join(lines[a - 1:b]) + "\n" + behind)
    src.append(EM.SHELL_TAIL)  # em_setup and the lists' text form
    src.append(TAIL)
    lib = os.path.join(tmp, "libcliquemergeprobe.so")
    subprocess.run(["g++", "-O1", "-std=c++14", "-w", "-fPIC", "-shared", f"-I{REF}", "-x", "c++", "-", "-o", lib], input="".join(src), text=True,
                   check=True)
    dll = C.CDLL(lib)
    dll.em_setup.restype = C.c_int
    dll.em_setup.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    dll.cm_clique.restype = C.c_int
    dll.cm_clique.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, C.c_uint64]
    return dll


def setup(dll, V, edges, reads, vertex_read, vertex_fwd, rng):
    """em_setup with distinct random mates; returns the lookup sequence -> (read, seq, rev)."""
    n, nr = len(edges), len(reads)
    arr = (EM.FragEdge * max(n, 1))()
    for k, (v1, v2, r1, r2, p1, p2, o1, o2, od) in enumerate(edges):
        arr[k] = EM.FragEdge(p1, p2, r1, r2, v1, v2, o1, o2, od, 0)
    rd = (EM.FragRead * max(nr, 1))()
    bases, quals, at, lookup = [], [], 0, {}
    rc = lambda s: "".join(EM.COMP[c] for c in reversed(s))  # noqa: E731
    for k, (l1, l2, p) in enumerate(reads):
        offs = []
        for mate, ln in ((1, l1), (2, l2)):
            s = "".join(rng.choice("ACGT") for _ in range(ln))
            while ln and (s in lookup or rc(s) in lookup):
                s = "".join(rng.choice("ACGT") for _ in range(ln))
            q = "".join(chr(rng.randrange(35, 74)) for _ in range(ln))
            if ln:
                seq_no = mate if p else 0
                lookup[s] = (k, seq_no, 0)
                lookup[rc(s)] = (k, seq_no, 1)
            bases.append(s)
            quals.append(q)
            offs.append(at)
            at += ln
        rd[k] = EM.FragRead(offs[0], offs[1], l1, l2, p)
    vr = np.asarray(vertex_read, np.uint32)
    vf = np.asarray(vertex_fwd, np.uint8)
    assert dll.em_setup(arr, n, V, rd, nr, "".join(bases).encode(), "".join(quals).encode(), vr.ctypes.data, vf.ctypes.data) == 0
    return lookup


def run_clique(dll, lookup, clique, m, ec):
    text = C.create_string_buffer(1 << 18)
    nodes = np.asarray(clique, np.uint32)
    assert dll.cm_clique(nodes.ctypes.data, nodes.size, m, ec, text, len(text)) == 0
    lines = text.value.decode().split("\n")
    typ, base, len1, len2, t1, t2, c1, c2 = lines[0].split()
    at, lists = 1, []
    for _ in range(2):
        cnt = int(lines[at])
        ent = []
        for ln in lines[at + 1:at + 1 + cnt]:
            pos, vertex, s, _q = ln.split()
            read, seq_no, rev = lookup[s]
            ent.append([read, seq_no, rev, int(pos), int(vertex), s])
        lists.append(ent)
        at += 1 + cnt
    for k in range(2):
        cnt = int(lines[at])
        if cnt < 0:  # not filtered: every member is used
            for e in lists[k]:
                e[5] = 1
            at += 1
            continue
        kept = {ln.split()[1] for ln in lines[at + 1:at + 1 + cnt]}
        n_used = 0
        for e in lists[k]:
            e[5] = 1 if e[5] in kept else 0
            n_used += e[5]
        assert n_used == cnt, "the filtered list is not the used members"
        at += 1 + cnt
    cnt = int(lines[at])
    subs = [[int(x) for x in ln.split()][1:] for ln in lines[at + 1:at + 1 + cnt]]
    assert cnt == len(clique)
    n_lay = 2 if typ == "p" else 1
    return dict(clique=list(clique), m=m, ec=ec, type=typ, base=int(base), total_len=[int(len1), int(len2)][:n_lay], trim=[int(t1), int(t2)],
                lists=lists[:n_lay], subreads=subs, _cons=[int(c1), int(c2)])


# ---- inputs ------------------------------------------------------------------------------------------------------------

def make_clique(b, rng, size, kinds, tie_heavy, far=False):
    """`size` fresh vertices; kinds: 's' all single-end, 'p' all paired, 'm' mixed.  Records base -> node or node -> base, positions from a
    range of +-tie_heavy where that is not 0 (equal positions and equal endpos), the base's read as read 1 or read 2.  far: a node beyond the base's end
    (an uncovered column).  The base is found as constructSuperread finds it."""
    vs = []
    for k in range(size):
        paired = {"s": 0, "p": 1, "m": int(rng.random() < 0.5)}[kinds]
        if kinds == "m" and k == size - 1 and all(b.reads[b.vread[v]][2] for v in vs):
            paired = 0  # a mixed clique has a single-end read
        if kinds == "m" and k == size - 2 and not any(b.reads[b.vread[v]][2] for v in vs):
            paired = 1
        lens = [50, 50] if tie_heavy else [rng.choice([40, 50, 55, 70]), rng.choice([35, 50, 64])]
        vs.append(b.vertex(paired, rng.random() < 0.6, lens[0], lens[1]))
    single = [v for v in vs if not b.reads[b.vread[v]][2]]
    base = single[0] if single else vs[0]
    typ_p = not single
    for v in vs:
        if v == base:
            continue
        span = tie_heavy or 30  # tie_heavy: the span itself
        pos1 = rng.randrange(-span, span + 1)
        pos2 = rng.randrange(-span, span + 1) if typ_p else rng.randrange(0, span + 1)
        if far and v == vs[-1] and v != base:
            pos1 = 200
        swap = rng.random() < 0.3
        od = rng.choice("12-")
        if rng.random() < 0.5:
            b.edge(base, v, pos1, pos2, od, swap)
            if rng.random() < 0.2:  # repeated: the first in list order wins
                b.edge(base, v, pos1 + 2, pos2, od, swap)
        else:
            b.edge(v, base, pos1, pos2, od, swap)
    order = list(vs)
    rng.shuffle(order)
    return order


def main():
    rng = random.Random(11)
    plan = []  # (size, m, ec, kinds, tie_heavy, far)
    for m in (1, 2, 4):
        for size in (3 * m, 3 * m + 1):
            for rep in range(4):
                for kinds in "spm":  # (the filtered ones of m = 2 and 4 all tie-heavy: endpos ties inside the cut group of a layout of at most 16)
                    plan.append((size, m, rep % 2, kinds, [2, 3, 4, 2][rep] if size > 3 * m and m > 1 else 4 * (rep >= 2), False))
    for rep in range(13):  # filtered layouts of more than 16 entries, two a clique
        plan.append((17, 4 if rep % 4 else 2, rep % 2, "p", 4 * (rep < 8), False))
    for rep in range(8):  # consensus returns -1 (too few members under error correction) and 0 (an uncovered column)
        plan.append((rng.choice([2, 3]), 4, 1, "sp"[rep % 2], False, False))
        plan.append((rng.choice([3, 5]), 2, rep % 2, "s", False, True))
    b = EM.Builder()
    cliques = [(make_clique(b, rng, size, kinds, tie, far), m, ec) for size, m, ec, kinds, tie, far in plan]
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        lookup = setup(dll, len(b.vread), b.edges, b.reads, b.vread, b.vfwd, rng)
        for clique, m, ec in cliques:
            cases.append(run_clique(dll, lookup, clique, m, ec))
    # what the file must hold, each at least a dozen times
    paired_of = lambda v: b.reads[b.vread[v]][2]  # noqa: E731
    count = dict(single=0, paired=0, mixed=0, fwd=0, rev=0, equal_pos=0, filt_small=0, filt_large=0, ret0=0, retm1=0, s_mate=0,
                 cut_tie_small=0, cut_tie_large=0, out_tie_small=0, out_tie_large=0)
    for q in cases:
        kinds = {paired_of(v) for v in q["clique"]}
        count["single" if kinds == {0} else "paired" if kinds == {1} else "mixed"] += 1
        count["fwd"] += sum(b.vfwd[v] for v in q["clique"])
        count["rev"] += sum(1 - b.vfwd[v] for v in q["clique"])
        for lst in q["lists"]:
            pos = [e[3] for e in lst]
            count["equal_pos"] += len(pos) != len(set(pos))
        if len(q["clique"]) > 3 * q["m"]:
            for lst in q["lists"]:
                lens = [b.reads[e[0]][1] if e[1] == 2 else b.reads[e[0]][0] for e in lst]
                end = [e[3] + ln for e, ln in zip(lst, lens)]
                small = len(lst) <= 16
                count["filt_small" if small else "filt_large"] += 1
                # the cut group: the smallest endpos among the vertices the walk added; a tie inside it that is not taken whole
                num = 2 * q["m"]
                first = {e[4] for e in lst[:num // 2]} | {q["base"]}
                added = [(en, e[4]) for e, en in zip(lst, end) if e[5] and e[4] not in first]
                if added:
                    cut = min(en for en, _ in added)
                    group = {e[4] for e, en in zip(lst, end) if en == cut and e[4] not in first}
                    taken = {v for en, v in added if en == cut}
                    # (a vertex of the group may have been taken through another entry with a larger endpos)
                    taken_elsewhere = {v for en, v in added if en > cut}
                    if group - taken - taken_elsewhere:
                        count["cut_tie_small" if small else "cut_tie_large"] += 1
                    elif len(end) != len(set(end)):
                        count["out_tie_small" if small else "out_tie_large"] += 1
            if q["type"] == "s":
                lst = q["lists"][0]
                for v in set(e[4] for e in lst):
                    if paired_of(v) and any(e[5] for e in lst if e[4] == v):
                        count["s_mate"] += 1
        count["ret0"] += sum(1 for t, n in zip(q["trim"][:len(q["lists"])], q["_cons"]) if t == 0 and n == 0)
        count["retm1"] += sum(1 for t in q["trim"][:len(q["lists"])] if t == -1)
    print(count)
    via_base = sum(1 for e in b.edges for q in cases if e[0] == q["base"] and e[1] in q["clique"])
    via_node = sum(1 for e in b.edges for q in cases if e[1] == q["base"] and e[0] in q["clique"])
    print("base -> node", via_base, "node -> base", via_node)
    assert all(v >= 12 for v in count.values()), count
    assert via_base >= 12 and via_node >= 12
    for m in (1, 2, 4):
        for size in (3 * m, 3 * m + 1):
            assert sum(1 for q in cases if q["m"] == m and len(q["clique"]) == size) >= 12, (m, size)
    for q in cases:
        del q["_cons"]
    # compact forms: vertex v reads read v (vertex_read is the identity) and a record's reads and orientations follow from its vertices
    assert b.vread == list(range(len(b.vread)))
    edges = []
    for v1, v2, r1, r2, p1, p2, o1, o2, od in b.edges:
        assert (o1, o2) == (b.vfwd[v1], b.vfwd[v2]) and {r1, r2} == {v1, v2}
        edges.append([v1, v2, p1, p2, od, int(r1 != v1)])
    doc = dict(note=PROVENANCE + ".  Vertex v reads read v.  edges = addEdge order, one record per entry: v1,v2,pos1,pos2,ord,swapped (1: read1 is "
                    "v2's read and read2 v1's; ori1 / ori2 = the vertices' orientations; score 1.0).  reads: len1,len2,paired per read.  cliques[]: the "
                    "clique as given, m = min_clique_size, ec = error_correction (minQual 0.99, subreads_needed false), type, base vertex, total_len "
                    "per layout ('l', 'r' or 's'), trim = trim_pos1, trim_pos2 (what consensus returned for the USED members), lists per layout in "
                    "list order: read, seq (0 | 1 | 2), rev, pos (shifted), vertex, used (1: handed to consensus; filter_subreads where the clique "
                    "is larger than 3 m); subreads: index1,startpos1,index2,startpos2 per clique vertex in ascending vertex order.",
               edges=edges, reads=b.reads, vertex_fwd=b.vfwd, cliques=cases)
    path = os.path.join(ROOT, "tests", "golden", "clique_merge.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    size = os.path.getsize(path)
    print(path, size, "bytes,", len(cases), "cliques")
    assert size <= 457014


if __name__ == "__main__":
    main()
