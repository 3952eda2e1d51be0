#!/usr/bin/env python3
"""Generates tests/golden/branch_reduce.json and tests/golden/evidence_threshold_table.tsv: what the reference's own second half of
BranchReduction::readBasedBranchReduction computes for the cases of tests/_branch_reduce.golden_cases.

Runs only in the build container (needs /root/reference).  A throw-away probe is compiled in a temporary directory from
src/BranchReduction.cpp:82-227 (behind a function head of this script's own: the lines start in the middle of readBasedBranchReduction),
:745-1291 and src/OverlapGraph.cpp:104-147, :233-259 (removeEdge, checkEdge), streamed from the reference by line range and never stored,
behind shells of this script's own, in the manner of make_golden_branch_evidence.py:
  - a declaration-only BranchReduction class with the members those lines use (all public);
  - a stand-in OverlapGraph with adj_out, adj_in, branching_edges, edge_count, getVertexCount and getEdgeInfo as src/OverlapGraph.cpp:263-282
    searches;
  - the genuine Read.h, Edge.h and Types.h.
The vectors are therefore "probe with substitutes".  The probe reads evidence_threshold_table.tsv from its working directory, as the
reference does.  Asserts are on: a case that trips one aborts the script.

Recorded per case: the inputs (tables), branching_components with dist, edges_to_remove (the records :217-225 appended, which are the sorted
list), the final adjacency (per record its target and pos2, which tells twins apart), branching_edges as (v1, v2), and the iteration orders
the probe's maps produced: branch_in_map's, branch_out_map's and, per component, unique_evidence_per_edge's — each from a map of the same
type that received the same inserts.  Recorded once: the iteration order of std::unordered_map< node_id_t, bool > for keys 0..40 inserted
ascending, which is what pins the file to a standard library.

The threshold table is the output of the reference's scripts/min_ev_table.py (-l 100 -i 20 -s 10 -c 30), run from its text with the three
Python 2 print statements turned into calls; nothing of it is stored.

    python tests/golden/make_golden_branch_reduce.py
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_self_overlap import REF, ROOT  # noqa: E402

sys.path.insert(0, ROOT)
from tests import _branch_reduce as T  # noqa: E402

HEAD = r"""
#include <assert.h>
#include <math.h>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "Types.h"
#include "Read.h"
#include "Edge.h"
struct Settings {
    bool verbose, careful, diploid;
    unsigned long original_readcount;
    double edge_threshold, merge_contigs;
};
class OverlapGraph {
public:
    std::vector< std::list< Edge > > adj_out;
    std::vector< std::list< node_id_t > > adj_in;
    std::vector< Edge > branching_edges;
    unsigned int edge_count;
    Settings program_settings;
    unsigned long getVertexCount() { return adj_out.size(); }
    Edge* getEdgeInfo(node_id_t v, node_id_t w, bool reverse_allowed) {
        for (auto it = adj_out.at(v).begin(); it != adj_out.at(v).end(); it++)
            if (it->get_vertex(2) == w) return &(*it);
        std::cerr << "Edge not found" << std::endl;
        exit(1);
    }
    Edge removeEdge(node_id_t v, node_id_t w);
    double checkEdge(node_id_t v, node_id_t w, bool reverse_allowed);
};
class BranchReduction {
public:
    std::shared_ptr<OverlapGraph> overlap_graph;
    Settings program_settings;
    std::vector< std::pair< std::vector< node_pair_t >, int > > branching_components;
    std::unordered_map< safe_edge_count_t, std::list< read_id_t > > evidence_per_edge;
    std::unordered_set< node_id_t > false_in_branches;
    std::unordered_set< node_id_t > false_out_branches;
    std::pair<int, node_id_t> extendComponentOut(std::vector< node_pair_t > & component, std::list< node_id_t > neighbors, bool & has_false_branch,
        std::unordered_map< node_id_t, bool > & visited_in_branches, std::unordered_map< node_id_t, bool > & visited_out_branches,
        std::unordered_map< node_id_t, std::list< node_id_t > > & branch_in_map, std::unordered_map< node_id_t, std::list< node_id_t > > & branch_out_map,
        std::unordered_map< node_id_t, int > & branch_out_dist_map);
    void extendComponentIn(std::vector< node_pair_t > & component, std::list< node_id_t > neighbors, bool & has_false_branch,
        std::unordered_map< node_id_t, bool > & visited_in_branches, std::unordered_map< node_id_t, bool > & visited_out_branches,
        std::unordered_map< node_id_t, std::list< node_id_t > > & branch_in_map, std::unordered_map< node_id_t, std::list< node_id_t > > & branch_out_map,
        std::unordered_map< node_id_t, int > & branch_out_dist_map);
    safe_edge_count_t edgeToEvidenceIndex(node_id_t node, node_id_t neighbor);
    node_pair_t evidenceIndexToEdge(safe_edge_count_t index);
    void findBranchingComponents(std::vector< std::pair< std::list< node_id_t >, int > > final_branch_in,
        std::vector< std::pair< std::list< node_id_t >, int > > final_branch_out, std::list< node_pair_t > & edges_to_remove);
    bool countUniqueEvidence(std::vector< node_pair_t > component, int min_evidence, std::list< node_pair_t > & edges_to_remove);
    void secondHalf(std::list< Edge > missing_edges, std::vector< std::pair< std::list< node_id_t >, int > > final_branch_in,
        std::vector< std::pair< std::list< node_id_t >, int > > final_branch_out);
};
"""

SECOND_HALF_HEAD = r"""
void BranchReduction::secondHalf(std::list< Edge > missing_edges, std::vector< std::pair< std::list< node_id_t >, int > > final_branch_in,
        std::vector< std::pair< std::list< node_id_t >, int > > final_branch_out) {
"""

DRIVER = r"""
template <class L> static void put_list(const L& l) {
    std::cout << "[";
    bool first = true;
    for (auto x : l) { std::cout << (first ? "" : ",") << x; first = false; }
    std::cout << "]";
}
int main() {
    unsigned long V, E, n_branches, n_ev, n_missing;
    int careful, diploid;
    auto graph = std::make_shared<OverlapGraph>();
    BranchReduction br;
    Settings ps;
    ps.verbose = false, ps.edge_threshold = 0.9, ps.merge_contigs = 0;
    std::cin >> V >> E >> n_branches >> n_ev >> n_missing >> careful >> diploid >> ps.original_readcount;
    ps.careful = careful != 0, ps.diploid = diploid != 0;
    graph->program_settings = ps, br.program_settings = ps, br.overlap_graph = graph;
    std::vector<Read> store;
    for (unsigned long r = 0; r < V; r++) {
        unsigned long len;
        std::cin >> len;
        store.push_back(Read(false, false, r, std::string(len, 'A'), "", std::string(len, 'I'), ""));
    }
    graph->adj_out.resize(V), graph->adj_in.resize(V), graph->edge_count = E;
    for (unsigned long k = 0; k < E; k++) {  // in sortAdjOut's order already (the first half ran it)
        unsigned long u, v;
        int pos1, pos2, len0;
        std::cin >> u >> v >> pos1 >> pos2 >> len0;
        Edge e(0.99, pos1, pos2, true, true, "-", &store.at(u), &store.at(v));
        e.set_vertices(u, v);
        e.set_len(len0, 0);
        graph->adj_out.at(u).push_back(e);
    }
    for (unsigned long v = 0; v < V; v++) {
        unsigned long n;
        std::cin >> n;
        for (unsigned long k = 0; k < n; k++) {
            unsigned long u;
            std::cin >> u;
            graph->adj_in.at(v).push_back(u);
        }
    }
    std::vector< std::pair< std::list< node_id_t >, int > > final_in(V, std::make_pair(std::list< node_id_t >(), 0)), final_out = final_in;
    std::unordered_map< node_id_t, std::list< node_id_t > > in_twin, out_twin;  // the inserts of :768 / :779
    for (unsigned long b = 0; b < n_branches; b++) {
        unsigned long node, n;
        int side, dist, is_false;
        std::cin >> node >> side >> dist >> is_false >> n;
        std::list< node_id_t > l;
        for (unsigned long k = 0; k < n; k++) {
            unsigned long x;
            std::cin >> x;
            l.push_back(x);
        }
        if (is_false) (side ? br.false_out_branches : br.false_in_branches).insert(node);
        if (n == 0) continue;
        (side ? out_twin : in_twin).insert(std::make_pair(node, l));
        l.push_front(node);
        (side ? final_out : final_in).at(node) = std::make_pair(l, dist);
    }
    for (unsigned long k = 0; k < n_ev; k++) {
        unsigned long u, v, n;
        std::cin >> u >> v >> n;
        std::list< read_id_t > l;
        for (unsigned long i = 0; i < n; i++) {
            unsigned long id;
            std::cin >> id;
            l.push_back(id);
        }
        br.evidence_per_edge.insert(std::make_pair(br.edgeToEvidenceIndex(u, v), l));
    }
    std::list< Edge > missing;
    for (unsigned long k = 0; k < n_missing; k++) {
        Edge e(0.97, 7 + k, 0, true, true, "-", &store.at(0), &store.at(0));
        e.set_vertices(k, k + 1);
        missing.push_back(e);
    }
    br.secondHalf(missing, final_in, final_out);
    std::cout << "{\"components\":[";
    for (size_t i = 0; i < br.branching_components.size(); i++) {
        std::cout << (i ? "," : "") << "[" << br.branching_components[i].second << ",[";
        for (size_t k = 0; k < br.branching_components[i].first.size(); k++)
            std::cout << (k ? "," : "") << "[" << br.branching_components[i].first[k].first << "," << br.branching_components[i].first[k].second << "]";
        std::cout << "]]";
    }
    std::cout << "],\"adj_out\":[";
    for (unsigned long v = 0; v < V; v++) {
        std::cout << (v ? "," : "") << "[";
        bool first = true;
        for (auto& e : graph->adj_out[v]) { std::cout << (first ? "" : ",") << "[" << e.get_vertex(2) << "," << e.get_pos(2) << "]"; first = false; }
        std::cout << "]";
    }
    std::cout << "],\"adj_in\":[";
    for (unsigned long v = 0; v < V; v++) { std::cout << (v ? "," : ""); put_list(graph->adj_in[v]); }
    std::cout << "],\"branching\":[";
    for (size_t k = 0; k < graph->branching_edges.size(); k++)
        std::cout << (k ? "," : "") << "[" << graph->branching_edges[k].get_vertex(1) << "," << graph->branching_edges[k].get_vertex(2) << "]";
    std::cout << "],\"edge_count\":" << graph->edge_count << ",\"orders\":[";
    {
        std::vector<node_id_t> a, b;
        for (auto& x : in_twin) a.push_back(x.first);
        for (auto& x : out_twin) b.push_back(x.first);
        put_list(a);
        std::cout << ",";
        put_list(b);
    }
    for (auto& comp : br.branching_components) {  // the inserts of :1040
        std::unordered_map< safe_edge_count_t, std::list< read_id_t > > twin;
        for (auto& p : comp.first) twin.insert(std::make_pair(br.edgeToEvidenceIndex(p.first, p.second), std::list< read_id_t >()));
        std::cout << ",[";
        bool first = true;
        for (auto& x : twin) { node_pair_t p = br.evidenceIndexToEdge(x.first); std::cout << (first ? "" : ",") << "[" << p.first << "," << p.second << "]"; first = false; }
        std::cout << "]";
    }
    std::cout << "],\"order41\":";
    {
        std::unordered_map< node_id_t, bool > m;
        for (node_id_t k = 0; k <= 40; k++) m.insert(std::make_pair(k, false));
        std::vector<node_id_t> a;
        for (auto& x : m) a.push_back(x.first);
        put_list(a);
    }
    std::cout << "}" << std::endl;
    return 0;
}
"""


def build_probe(tmp):
    br = open(os.path.join(REF, "BranchReduction.cpp")).read().split("\n")
    og = open(os.path.join(REF, "OverlapGraph.cpp")).read().split("\n")
    src = os.path.join(tmp, "branch_reduce.cpp")
    with open(src, "w") as f:
        f.write(HEAD)
        f.write("\n".join(og[103:147]) + "\n" + "\n".join(og[232:259]) + "\n")
        f.write(SECOND_HALF_HEAD + "\n".join(br[80:227]) + "\n")
        f.write("\n".join(br[744:1291]) + "\n")
        f.write(DRIVER)
    exe = os.path.join(tmp, "branch_reduce")
    subprocess.run(["g++", "-std=c++11", "-O1", "-w", "-I", REF, "-o", exe, src], check=True)  # (no -DNDEBUG: the asserts are on)
    return exe


def probe_input(case):
    g = case.graph()
    V = case.n_vertices
    t = [V, g["edges"].size, len(case.branches), len(case.evidence), case.n_missing, case.careful, case.diploid, case.original_readcount]
    t += case.read_len
    for u in range(V):  # sortAdjOut: short lists, so std::sort is an insertion sort and stable
        recs = g["edges"][int(g["out_off"][u]):int(g["out_off"][u + 1])]
        for e in recs[np.argsort(recs["v2"], kind="stable")]:
            t += [int(e["v1"]), int(e["v2"]), int(e["pos1"]), int(e["pos2"]), int(e["len0"])]
    for v in range(V):
        l = g["in_nodes"][int(g["in_off"][v]):int(g["in_off"][v + 1])]
        t += [len(l)] + [int(x) for x in l]
    for node, side, dist, is_false, final in case.branches:
        t += [node, side, dist, is_false, len(final)] + list(final)
    for (u, v), ids in sorted(case.evidence.items()):
        t += [u, v, len(ids)] + list(ids)
    return " ".join(str(x) for x in t) + "\n"


def run_case(exe, tmp, case):
    assert max(len([1 for e in case.edges if e[0] == u]) for u in range(case.n_vertices)) <= 16
    open(os.path.join(tmp, "evidence_threshold_table.tsv"), "w").write(case.table_text())
    r = subprocess.run([exe], input=probe_input(case), capture_output=True, text=True, cwd=tmp)
    assert r.returncode == 0, (case.name, r.returncode, r.stderr[-2000:])  # an assert or exit of the reference: not a case to record
    ref = json.loads(r.stdout[r.stdout.index('{"components"'):])  # (the reference prints "conflict - 2 supported edges" and the like)
    n_removed = len(ref["branching"]) - case.n_missing
    assert ref["edge_count"] == len(case.edges) - n_removed
    want = dict(components=ref["components"], removed=ref["branching"][case.n_missing:], adj_out=ref["adj_out"], adj_in=ref["adj_in"], branching=ref["branching"])
    if case.spec:  # the tables are tests/_branch_reduce.double_branch's: recorded as its arguments
        n, counts, dip = case.spec
        assert T.double_branch(case.name, counts, n, diploid=dip).to_json() == case.to_json()
        return [case.name, case.spec] + [want[k] for k in T.WANT_KEYS] + [ref["orders"]], ref["order41"]
    return [case.name, case.to_json()] + [want[k] for k in T.WANT_KEYS] + [ref["orders"]], ref["order41"]


def threshold_table(tmp):
    text = open(os.path.join(os.path.dirname(REF), "scripts", "min_ev_table.py")).read()
    text = re.sub(r"^(\s*)print (.+)$", r"\1print(\2)", text, flags=re.M)
    out = os.path.join(tmp, "table.tsv")
    argv, sys.argv = sys.argv, ["min_ev_table.py", "-l", "100", "-i", "20", "-s", "10", "-c", "30", "-o", out]
    try:
        exec(compile(text + "\nmain()\n", "min_ev_table.py", "exec"), {"__name__": "min_ev_table"})
    finally:
        sys.argv = argv
    return open(out).read()


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_probe(tmp)
        done = [run_case(exe, tmp, c) for c in T.golden_cases()]
        table = threshold_table(tmp)
    cases, order41 = [d[0] for d in done], done[0][1]
    assert all(d[1] == order41 for d in done)
    in_order = next(c for c in cases if c[0] == "rehash")[-1][0]
    assert len(in_order) >= 30 and in_order[0] not in (min(in_order), max(in_order)), in_order[0]
    assert in_order.index(9) < in_order.index(5)
    out = dict(provenance="probe with substitutes: src/BranchReduction.cpp:82-227, :745-1291 and src/OverlapGraph.cpp:104-147, :233-259 with the genuine Read.h / "
                          "Edge.h / Types.h, a declaration-only BranchReduction and a stand-in OverlapGraph; built with g++ against libstdc++",
               unordered_map_order_0_40=order41, case_fields=["name", "inputs, or [n_edges, counts, diploid] of double_branch"] + list(T.WANT_KEYS) + ["orders"],
               cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "branch_reduce.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    tpath = os.path.join(ROOT, "tests", "golden", "evidence_threshold_table.tsv")
    open(tpath, "w").write(table)
    print(f"{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}; {len(table.splitlines())} lines -> {tpath}")


if __name__ == "__main__":
    main()
