#!/usr/bin/env python3
"""Generates tests/golden/originals.json: the original-read index maps the reference's own statements build, the lines its writer writes
for them and what its reader makes of those lines.

Runs only in the build container (needs /root/reference).  The probes are compiled in a temporary directory from line ranges streamed from
the reference and are never stored:

(a) src/SRBuilder.cpp:750-843, constructSuperread's loop over a clique's vertices and their originals (the lines behind :806 are comments
    and the loop's brace), in a function of the probe's own that declares what the lines before :750 declare: the sorted clique,
    subreads_map, len2, program_settings.first_it, and stand-ins for OverlapGraph (vertex_to_read, getOrientation, original_ID_dict) and
    FastqStorage (get_read) over the genuine Read.h and Types.h;
(b) :938-949, merge_self_overlap's shift, on the map of (a);
(c) :1180-1218, the forward and the reverse branch of a trivial super-read;
(d) :1449-1463, the writer's lines, on every map of (a) - (c), and src/OverlapGraph.cpp:805-838, buildOriginalsDict's reader, on those
    lines, with a few-line stand-in for boost::algorithm::split / is_any_of / token_compress_on (adjacent separators are one; an empty
    token where the field begins or ends with a separator).
The vectors are therefore "probe with substitutes".

A case is one iteration's worth of tables as tests/_originals.make_case builds them (a dict, super-reads over sorted vertex samples, the
trivials, the new ids); each super-read and each trivial goes through the probes on its own.  Only inputs on which the reference neither
asserts nor reads a field it never set: no single-end original in a paired read under a reverse vertex (:801), no read without an original (:1178), index2 /
len2 of a single-end original given as 0 and recorded for paired originals only.  Maps are recorded as lists sorted by original id; the
lines as the reference wrote them (their order inside a line is libstdc++'s unordered_map's: the tests compare a line as a set of fields).

    python tests/golden/make_golden_originals.py
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_self_overlap import REF, ROOT  # noqa: E402

sys.path.insert(0, ROOT)
from haploconduct_amd import merge_next as MN  # noqa: E402
from tests import _originals as O  # noqa: E402

HEAD = r"""
#include <assert.h>
#include <string.h>
#include <algorithm>
#include <deque>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "Read.h"
#include "Types.h"
namespace boost {
struct any_of_t {
    std::string set;
    bool operator()(char c) const { return set.find(c) != std::string::npos; }
};
inline any_of_t is_any_of(const char* s) { return any_of_t{s}; }
enum token_compress_mode_type { token_compress_on, token_compress_off };
namespace algorithm {
template <class V, class P>
void split(V& out, const std::string& in, P pred, token_compress_mode_type mode) {
    out.clear();
    std::string cur;
    for (size_t i = 0; i < in.size(); i++) {
        if (pred(in[i])) {
            out.push_back(cur);
            cur.clear();
            if (mode == token_compress_on)
                while (i + 1 < in.size() && pred(in[i + 1])) i++;
        } else {
            cur.push_back(in[i]);
        }
    }
    out.push_back(cur);
}
}
}
typedef std::unordered_map< read_id_t, OriginalIndex > Map;
struct Graph {
    std::vector<read_id_t> vertex_to_read;
    std::vector<int> ori;
    std::unordered_map< read_id_t, Map > original_ID_dict;
    bool getOrientation(node_id_t v) { return ori.at(v) != 0; }
};
struct Storage {
    std::vector<Read> reads;
    Read* get_read(read_id_t i) { return &reads.at(i); }
};
// an entry: id, index1, index2, len1, len2, paired, forward
static Map to_map(const long* e, long n) {
    Map m;
    for (long i = 0; i < n; i++, e += 7) {
        OriginalIndex x;
        x.index1 = e[1], x.index2 = e[2], x.len1 = (int)e[3], x.len2 = (int)e[4], x.is_paired = e[5] != 0, x.forward = e[6] != 0;
        m.insert(std::make_pair((read_id_t)e[0], x));
    }
    return m;
}
static int from_map(const Map& m, long* out) {
    std::vector<read_id_t> ids;
    for (auto it : m) ids.push_back(it.first);
    std::sort(ids.begin(), ids.end());
    for (read_id_t id : ids) {
        const OriginalIndex& x = m.at(id);
        out[0] = (long)id, out[1] = x.index1, out[3] = x.len1, out[5] = x.is_paired, out[6] = x.forward;
        out[2] = x.is_paired ? x.index2 : 0;  // (never set for a single-end original)
        out[4] = x.is_paired ? x.len2 : 0;
        out += 7;
    }
    return (int)ids.size();
}
static int finish(const Map& result, read_id_t ID, long* out, char* line, long cap) {
    std::deque<Read> vec;
    Read holder(false, true, ID, "A", "", "I", "");
    holder.set_original_reads(result);
    vec.push_back(holder);
    std::deque<Read>::const_iterator it = vec.begin();
    std::ostringstream originals;
    std::string ori;
    int len1;
"""
FINISH_TAIL = r"""
    const std::string s = originals.str();
    if ((long)s.size() + 1 > cap) return -1;
    memcpy(line, s.c_str(), s.size() + 1);
    return from_map(result, out);
}
extern "C" int probe_construct(const unsigned long* clique_in, int n_clique, const unsigned long* v2r, const int* ori_in, int nv, const int* read_paired,
                               const int* read_len1, const int* read_len2, int n_reads, const long* dict_off, const long* dict_entries, const int* sub,
                               int first_it, int len2_in, int overlap_pos, int seq1_len, unsigned long new_id, long* out, char* line, long cap) {
    Graph graph;
    Graph* overlap_graph = &graph;
    graph.vertex_to_read.assign(v2r, v2r + nv);
    graph.ori.assign(ori_in, ori_in + nv);
    Storage storage;
    Storage* fastq_storage = &storage;
    for (int r = 0; r < n_reads; r++) {
        graph.original_ID_dict.insert(std::make_pair((read_id_t)r, to_map(dict_entries + 7 * dict_off[r], dict_off[r + 1] - dict_off[r])));
        const std::string s1(read_len1[r], 'A'), s2(read_paired[r] ? read_len2[r] : 0, 'C');
        storage.reads.push_back(Read(read_paired[r] != 0, false, r, s1, s2, std::string(s1.size(), 'I'), std::string(s2.size(), 'I')));
    }
    struct { bool first_it; } program_settings = {first_it != 0};
    std::vector< node_id_t > clique(clique_in, clique_in + n_clique);
    std::unordered_map< node_id_t, SubreadInfo > subreads_map;
    for (int i = 0; i < n_clique; i++) {
        SubreadInfo s;
        s.index1 = sub[4 * i], s.index2 = sub[4 * i + 1], s.startpos1 = sub[4 * i + 2], s.startpos2 = sub[4 * i + 3];
        subreads_map.insert(std::make_pair(clique[i], s));
    }
    int len2 = len2_in;
"""
CONSTRUCT_MID = r"""
    Map result = original_reads;
    if (overlap_pos >= 0) {
        Read superread(true, true, new_id, std::string(seq1_len, 'A'), "C", std::string(seq1_len, 'I'), "I");
        superread.set_original_reads(original_reads);
        Read merged_superread(false, true, new_id, "A", "", "I", "");
        std::string seq1 = superread.get_seq(1);
"""
CONSTRUCT_TAIL = r"""
        result = merged_superread.get_original_reads();
    }
    return finish(result, new_id, out, line, cap);
}
extern "C" int probe_trivial(int paired, int len1_in, int len2_in, int fwd, const long* entries, long n, unsigned long new_id, long* out, char* line,
                             long cap) {
    Graph graph;
    Graph* overlap_graph = &graph;
    graph.ori.push_back(fwd);
    node_id_t v = 0;
    const std::string s1(len1_in, 'A'), s2(paired ? len2_in : 0, 'C');
    Read the_read(paired != 0, false, 5, s1, s2, std::string(s1.size(), 'I'), std::string(s2.size(), 'I'));
    Read* read = &the_read;
    read_id_t count = new_id;
    Map subreads = to_map(entries, n);
    std::deque<Read> trivial_SR_vec;
"""
TRIVIAL_TAIL = r"""
    return finish(trivial_SR_vec.back().get_original_reads(), new_id, out, line, cap);
}
extern "C" int probe_parse(const char* text, unsigned long id_wanted, long* out, long* n_lines) {
    Graph graph;
    std::unordered_map< read_id_t, Map >& original_ID_dict = graph.original_ID_dict;
    std::istringstream originals(text);
    std::string line;
    std::stringstream ss;
"""
PARSE_TAIL = r"""
    *n_lines = (long)original_ID_dict.size();
    auto f = original_ID_dict.find(id_wanted);
    if (f == original_ID_dict.end()) return -1;
    return from_map(f->second, out);
}
"""


def build_probe(tmp):
    src = os.path.join(tmp, "originals.cpp")
    sr = open(os.path.join(REF, "SRBuilder.cpp")).read().split("\n")
    og = open(os.path.join(REF, "OverlapGraph.cpp")).read().split("\n")
    with open(src, "w") as f:
        f.write(HEAD)
        f.write("\n".join(sr[1448:1463]) + "\n")
        f.write(FINISH_TAIL)
        f.write("\n".join(sr[749:843]) + "\n")
        f.write(CONSTRUCT_MID)
        f.write("\n".join(sr[937:949]) + "\n")
        f.write(CONSTRUCT_TAIL)
        f.write("\n".join(sr[1179:1218]) + "\n")
        f.write(TRIVIAL_TAIL)
        f.write("\n".join(og[804:838]) + "\n")
        f.write(PARSE_TAIL)
    so = os.path.join(tmp, "originals.so")
    subprocess.run(["g++", "-std=c++11", "-O1", "-fPIC", "-shared", "-w", "-I", REF, "-o", so, src], check=True)
    dll = C.CDLL(so)
    vp = C.c_void_p
    dll.probe_construct.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulong, vp, vp, C.c_long]
    dll.probe_trivial.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_long, C.c_ulong, vp, vp, C.c_long]
    dll.probe_parse.argtypes = [C.c_char_p, C.c_ulong, vp, vp]
    return dll


# seed, n_vertices, super-read sizes, keywords of tests/_originals.make_case (never wide or empty, seq0 only as "fwd": see above)
CASES = [
    ("first_it_pairs", 101, 14, [2, 2, 2, 2], dict(first_it=True, dict_sizes=(1,))),
    ("first_it_cliques", 102, 30, [3, 3, 5, 2, 7], dict(first_it=True, dict_sizes=(1,))),
    ("first_it_40", 103, 60, [40, 3], dict(first_it=True, dict_sizes=(1,))),
    ("later_pairs", 104, 16, [2, 2, 2, 2, 2], dict(dict_sizes=(1, 2))),
    ("later_pairs_shared", 105, 16, [2, 2, 2, 2, 2], dict(dict_sizes=(1, 2, 3), n_orig=6)),
    ("later_all_share", 108, 20, [3, 3, 2], dict(share=True, dict_sizes=(4,))),
    ("later_40", 109, 70, [40, 2], dict(dict_sizes=(1, 2), n_orig=90)),
    ("later_dict65", 110, 7, [3, 2], dict(dict_sizes=(1, 2, 65), n_orig=300)),
] + [(f"later_seed{s}", s, 24, [2, 3, 2, 3, 4], dict(dict_sizes=(1, 2, 3), n_orig=30, seq0="fwd" if s % 2 else False)) for s in range(120, 124)]

COVER = ("clique2", "clique3", "clique40", "dict1", "dict2", "dict65", "shared", "orig_p_sub_p", "orig_p_sub_s", "orig_s_sub_s", "orig_s_sub_p_fwd",
         "fwd", "rev", "first_it", "later", "s", "p", "self", "dummy", "negative", "len2_zero", "trivial_fwd_single", "trivial_rev_single",
         "trivial_fwd_paired", "trivial_rev_paired", "trivial_rev_single_paired_original")


def rows_of(buf, n):
    """7 longs per entry -> [id, forward, index1, len1] or [id, forward, index1, len1, index2, len2]"""
    out = []
    for i in range(n):
        oid, i1, i2, l1, l2, p, f = (int(buf[7 * i + k]) for k in range(7))
        out.append([oid, f, i1, l1, i2, l2] if p else [oid, f, i1, l1])
    return out


def rows_of_map(m):
    return [[oid, int(e["forward"]), e["index1"], e["len1"]] + ([e["index2"], e["len2"]] if e["paired"] else []) for oid, e in sorted(m.items())]


def flat(m):
    out = []
    for oid, e in sorted(m.items()):
        out += [oid, e["index1"], e["index2"], e["len1"], e["len2"], int(e["paired"]), int(e["forward"])]
    return out


def run_case(dll, name, seed, nv, sizes, kw):
    maps, t = O.make_case(seed, nv, sizes, **kw)
    n_reads, n_new = len(maps), int(t.new_read_count)
    al = lambda x: (C.c_long * max(1, len(x)))(*x)
    ai = lambda x: (C.c_int * max(1, len(x)))(*x)
    aul = lambda x: (C.c_ulong * max(1, len(x)))(*x)
    dict_off, dict_entries = [0], []
    for m in maps:
        dict_entries += flat(m)
        dict_off.append(len(dict_entries) // 7)
    read_of = {int(t.vertex_read[v]): v for v in range(nv)}
    read_paired = [int(t.nodes[read_of[r]]["paired"]) for r in range(n_reads)]
    read_len1 = [int(t.nodes[read_of[r]]["len1"]) for r in range(n_reads)]
    read_len2 = [int(t.nodes[read_of[r]]["len2"]) for r in range(n_reads)]
    cap = 1 << 20
    line = C.create_string_buffer(cap)
    want, lines, cover = [None] * n_new, [None] * n_new, set()
    cover.add("first_it" if t.first_it else "later")
    for k, c in enumerate(int(x) for x in t.sr_clique):
        a, b = int(t.subread_off[k]), int(t.subread_off[k + 1])
        rows = t.subreads[a:b]
        merged = t.kind[c] == MN.MN_SINGLE_SELF
        op = int(t.overlap_pos[c]) if merged else -1
        two = int(t.first_layout[c + 1]) - int(t.first_layout[c]) == 2
        len2 = int(t.layouts[int(t.first_layout[c]) + 1]["total_len"]) if two else 0
        sub = []
        for row in rows:
            i2 = int(row["index2"])
            sub += [int(row["index1"]), i2 - op if merged and i2 >= 0 else i2, int(row["startpos1"]), int(row["startpos2"])]
        clique = [int(x) for x in rows["node"]]
        assert clique == sorted(clique)
        total = sum(len(maps[int(t.vertex_read[v])]) for v in clique)
        out = (C.c_long * (7 * max(1, total)))()
        nid = int(t.new_id[c])
        n = dll.probe_construct(aul(clique), len(clique), aul([int(x) for x in t.vertex_read]), ai([int(x) for x in t.vertex_fwd]), nv, ai(read_paired),
                                ai(read_len1), ai(read_len2), n_reads, al(dict_off), al(dict_entries), ai(sub), int(t.first_it), len2, op, 150, nid, out, line,
                                cap)
        assert 0 <= n <= total, (name, k, n)
        want[nid], lines[nid] = rows_of(out, n), line.value.decode()
        # what the case covers
        cover |= {f"clique{len(clique)}"} & set(COVER)
        cover.add("p" if two else "s")
        ids = [oid for v in clique for oid in maps[int(t.vertex_read[v])]]
        if len(ids) != len(set(ids)):
            cover.add("shared")
        if merged:
            cover.add("self")
        if two and len2 == 0:
            cover.add("len2_zero")
        for v, row in zip(clique, rows):
            m = maps[int(t.vertex_read[v])]
            cover |= {f"dict{len(m)}"} & set(COVER)
            cover.add("fwd" if t.vertex_fwd[v] else "rev")
            if row["index2"] < 0:
                cover.add("dummy")
            for e in m.values():
                sp = bool(t.nodes[v]["paired"])
                if not e["paired"] and sp:
                    assert t.first_it or t.vertex_fwd[v], "the :801 assert: make_case must not build this"
                    cover.add("orig_s_sub_p_fwd")
                else:
                    cover.add(f"orig_{'p' if e['paired'] else 's'}_sub_{'p' if sp else 's'}")
        if any(r[2] < 0 or (len(r) == 6 and r[4] < 0) for r in want[nid]):
            cover.add("negative")
    for v in range(nv):
        if t.vertex_state[v] != MN.MN_V_TRIVIAL:
            continue
        node, m = t.nodes[v], maps[int(t.vertex_read[v])]
        assert m, "the :1178 assert: make_case must not build this"
        out = (C.c_long * (7 * len(m)))()
        nid = int(node["id"])
        n = dll.probe_trivial(int(node["paired"]), int(node["len1"]), int(node["len2"]), int(t.vertex_fwd[v]), al(flat(m)), len(m), nid, out, line, cap)
        assert n == len(m)
        want[nid], lines[nid] = rows_of(out, n), line.value.decode()
        cover.add(f"trivial_{'fwd' if t.vertex_fwd[v] else 'rev'}_{'paired' if node['paired'] else 'single'}")
        if not t.vertex_fwd[v] and not node["paired"] and any(e["paired"] for e in m.values()):
            cover.add("trivial_rev_single_paired_original")
    assert all(w is not None for w in want), name
    assert all(l.endswith("\n") and l.count("\n") == 1 and l[:-1].split("\t")[0] == str(r) for r, l in enumerate(lines)), name
    # buildOriginalsDict's reader on the whole file the writers made
    text = "".join(lines).encode()
    parsed = []
    nl = C.c_long()
    for r in range(n_new):
        out = (C.c_long * (7 * max(1, len(want[r]))))()
        n = dll.probe_parse(text, r, out, C.byref(nl))
        assert n == len(want[r]) and nl.value == n_new, (name, r, n)
        parsed.append(rows_of(out, n))
    assert parsed == want, name  # (the reference reads back what it wrote)
    nodes = [[int(x["len1"]), int(x["len2"]), int(x["paired"])] for x in t.nodes]
    tables = dict(kind=t.kind.tolist(), new_id=t.new_id.tolist(), overlap_pos=t.overlap_pos.tolist(), first_layout=t.first_layout.tolist(),
                  layouts=[[int(x["first_member"]), int(x["n_members"]), int(x["total_len"])] for x in t.layouts], sr_clique=t.sr_clique.tolist(),
                  subread_off=t.subread_off.tolist(), subreads=[[int(x[k]) for k in ("node", "index1", "index2", "startpos1", "startpos2")] for x in t.subreads],
                  vertex_state=t.vertex_state.tolist(), nodes=nodes, trivial_id=[[v, int(t.nodes[v]["id"])] for v in range(nv) if t.vertex_state[v] == MN.MN_V_TRIVIAL],
                  vertex_read=t.vertex_read.tolist(), vertex_fwd=t.vertex_fwd.tolist(), new_read_count=n_new, first_it=int(t.first_it))
    # (parsed is not stored: it equals want, asserted above)
    return dict(name=name, tables=tables, dict=[rows_of_map(m) for m in maps], want=want, lines=[l[:-1] for l in lines], covers=sorted(cover))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_probe(tmp)
        cases = [run_case(dll, *c) for c in CASES]
    seen = set(x for c in cases for x in c["covers"])
    assert seen >= set(COVER), set(COVER) - seen
    out = dict(provenance="probe with substitutes: src/SRBuilder.cpp:750-843, :938-949, :1180-1218, :1449-1463 and src/OverlapGraph.cpp:805-838 with the "
                          "genuine Read.h / Types.h, stand-ins for OverlapGraph, FastqStorage and boost::algorithm::split",
               entry="[id, forward, index1, len1] or, paired, [id, forward, index1, len1, index2, len2]", required_cover=list(COVER), cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "originals.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(f"{len(cases)} cases, {sum(len(c['want']) for c in cases)} new reads, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
