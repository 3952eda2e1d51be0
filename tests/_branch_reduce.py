"""Shared by the branch-reduction tests and tests/golden/make_golden_branch_reduce.py: cases given as the TABLES the second half of
BranchReduction::readBasedBranchReduction starts from (reference src/BranchReduction.cpp:82-227, :745-1272) — a graph, per branch its
final_branch and dist, evidence_per_edge, the missing edges, the threshold table —, a Python RESTATEMENT of the cited lines that takes the
iteration order of the reference's unordered_maps as an argument, and the comparison of a BranchReduction with it.

The restatement is written from the cited lines with Python lists and dicts; it is not the reference (the golden file is) but a second
reading of it.  Where the reference iterates an unordered_map the restatement asks `orders`: the recorded order reproduces libstdc++, any
other order (ascending, say) shows what would change."""
import json
import os
from dataclasses import dataclass, field

import numpy as np

from haploconduct_amd import branch_evidence as BR
from haploconduct_amd.host import EDGE_DTYPE
from haploconduct_amd.readstore import ReadSet

IN, OUT = BR.BR_IN, BR.BR_OUT


@dataclass
class Case:
    """Vertex v is read v, single-end, read_len[v] bases.  edges: (u, v, len0) in adj_out order per u; adj_in is in the order of the edges
    unless in_lists says otherwise.  branches: (node, side, dist, is_false, [final_branch neighbours]) — in-branches in ascending vertex, then
    out-branches.  evidence: {(u, v): ascending ids}; every final_branch edge has a key unless the case is about the missing one."""
    name: str
    read_len: list
    edges: list
    branches: list
    evidence: dict
    thresholds: dict
    careful: int = 0
    diploid: int = 1
    original_readcount: int = 1000
    n_missing: int = 0
    in_lists: dict = None
    spec: list = None         # [n_edges, counts, diploid] of a plain double_branch case: the golden file records that in place of the tables

    @property
    def n_vertices(self):
        return len(self.read_len)

    def reads(self):
        off = np.zeros(self.n_vertices + 1, np.uint64)
        off[1:] = np.cumsum(self.read_len)
        bases = np.full(int(off[-1]), ord("A"), np.uint8)
        return ReadSet(bases, np.full(bases.size, ord("I"), np.uint8), off, np.arange(self.n_vertices + 1, dtype=np.uint32), np.arange(self.n_vertices, dtype=np.uint64))

    def graph(self):
        V = self.n_vertices
        by_u = [[] for _ in range(V)]
        for u, v, l0 in self.edges:
            by_u[u].append((v, l0))
        recs = [(u, v, l0) for u in range(V) for v, l0 in by_u[u]]
        out_off = np.zeros(V + 1, np.uint64)
        out_off[1:] = np.cumsum([len(l) for l in by_u])
        edges = np.zeros(len(recs), EDGE_DTYPE)
        for k, (u, v, l0) in enumerate(recs):
            e = edges[k]
            e["score"], e["mismatch_rate"], e["pos1"], e["pos2"] = 0.99, 0.0, self.read_len[u] - l0, k  # (pos2 = k tells twins apart)
            e["ori1"], e["ori2"], e["ord"], e["read1"], e["read2"], e["v1"], e["v2"] = 1, 1, ord("-"), u, v, u, v
            e["perc"], e["len0"], e["len1"] = 50, l0, l0
        ins = [[] for _ in range(V)]
        for u, v, _ in recs:
            ins[v].append(u)
        for v, l in (self.in_lists or {}).items():
            assert sorted(l) == sorted(ins[v])
            ins[v] = list(l)
        in_off = np.zeros(V + 1, np.uint64)
        in_off[1:] = np.cumsum([len(l) for l in ins])
        return dict(edges=edges, out_off=out_off, in_nodes=np.array([u for l in ins for u in l], np.uint32), in_off=in_off)

    def missing(self):
        m = np.zeros(self.n_missing, EDGE_DTYPE)
        for k in range(self.n_missing):
            m[k]["score"], m[k]["mismatch_rate"], m[k]["v1"], m[k]["v2"], m[k]["pos1"], m[k]["ord"] = 0.97, -1.0, k, k + 1, 7 + k, ord("-")
        return m

    def tables(self):
        """a branch_evidence.BranchEvidence as hc_br_evidence_fetch would fill it"""
        b = np.zeros(len(self.branches), BR.BRANCH_DTYPE)
        nb = []
        for k, (node, side, dist, is_false, final) in enumerate(self.branches):
            b[k]["node"], b[k]["side"], b[k]["is_false"], b[k]["dist"], b[k]["nb_first"], b[k]["nb_count"] = node, side, is_false, dist, len(nb), len(final)
            b[k]["n_neighbours"] = max(len(final), 2)
            nb += final
        keys = sorted(self.evidence)
        off = np.zeros(len(keys) + 1, np.uint64)
        off[1:] = np.cumsum([len(self.evidence[k]) for k in keys])
        ids = np.array([i for k in keys for i in self.evidence[k]], np.uint32)
        return BR.BranchEvidence(b, np.array(nb, np.uint32), np.zeros(0, np.int32), np.array(keys, np.uint32).reshape(-1, 2), off, ids, self.missing(), {})

    def settings(self):
        return BR.reduce_settings(self.thresholds, careful=self.careful, diploid=self.diploid)

    def table_text(self):
        return "# dist\texp_ev\tmin_ev\n" + "".join(f"{d}\t0\t{m}\n" for d, m in sorted(self.thresholds.items()))

    def to_json(self):
        return dict(name=self.name, read_len=self.read_len, edges=[list(e) for e in self.edges], branches=[[n, s, d, f, list(l)] for n, s, d, f, l in self.branches],
                    evidence=[[u, v, list(ids)] for (u, v), ids in sorted(self.evidence.items())], thresholds=_runs(self.thresholds), careful=self.careful,
                    diploid=self.diploid, original_readcount=self.original_readcount, n_missing=self.n_missing,
                    in_lists={str(k): v for k, v in (self.in_lists or {}).items()})

    @classmethod
    def from_json(cls, j):
        return cls(j["name"], j["read_len"], [tuple(e) for e in j["edges"]], [(n, s, d, f, list(l)) for n, s, d, f, l in j["branches"]],
                   {(u, v): ids for u, v, ids in j["evidence"]}, {d: m for lo, hi, m in j["thresholds"] for d in range(lo, hi + 1)}, j["careful"], j["diploid"],
                   j["original_readcount"], j["n_missing"], {int(k): v for k, v in j["in_lists"].items()} or None)


def _runs(thresholds):
    """{dist: min_evidence} as [first dist, last dist, min_evidence] runs"""
    out = []
    for d, m in sorted(thresholds.items()):
        if out and out[-1][1] == d - 1 and out[-1][2] == m:
            out[-1][1] = d
        else:
            out.append([d, d, m])
    return out


def build(name, V, edges, counts=None, read_len=200, len0=120, dist=100, false=(), drop=(), cleared=(), shared=(), **kw):
    """A case from a graph: every vertex with more than one in- / out-neighbour is a branch over its ascending neighbours.  edges: (u, v) or
    (u, v, len0).  counts: {(u, v): n} private ids per edge (default 3); shared: [(id, [(u, v), ...])] ids that several edges list.  dist: one
    value or {(node, side): value}.  false: {(node, side)}; drop: {(node, side, neighbour)} leaves that branch's final_branch only; cleared:
    {(node, side)} branches whose final_branch :330-332 cleared."""
    edges = [(e[0], e[1], e[2] if len(e) > 2 else len0) for e in edges]
    lens = read_len if isinstance(read_len, list) else [read_len] * V
    ins, outs = [[] for _ in range(V)], [[] for _ in range(V)]
    for u, v, _ in edges:
        ins[v].append(u), outs[u].append(v)
    branches, ev = [], {}
    for side, lists in ((IN, ins), (OUT, outs)):
        for node in range(V):
            if len(lists[node]) < 2:
                continue
            final = [] if (node, side) in cleared else [x for x in sorted(set(lists[node])) if (node, side, x) not in drop]
            d = dist.get((node, side), 100) if isinstance(dist, dict) else dist
            branches.append((node, side, d, int((node, side) in false), final))
            for x in final:
                ev[(x, node) if side == IN else (node, x)] = []
    next_id = 0
    for key in sorted(ev):
        n = (counts or {}).get(key, 3)
        ev[key] = list(range(next_id, next_id + n))
        next_id += n + 5
    for i, keys in shared:
        for key in keys:
            ev[key] = sorted(ev[key] + [next_id + i])
    kw.setdefault("thresholds", {d: 2 for d in range(100, 200)})
    return Case(name, lens, edges, branches, ev, **kw)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

class Ends(Exception):
    """where the reference ends (exit(1), an exception nobody catches, undefined behaviour)"""


def ascending(keys):
    return sorted(keys)


def restate(case, order=ascending):
    """:82-227 with :745-1272.  order(keys in insertion order) -> the iteration order of an unordered_map that received them.  Returns
    dict(components=[(dist, [(u, v)])], removed=[(u, v)], adj_out=[[v]], adj_in=[[u]], branching=[(v1, v2)])."""
    V = case.n_vertices
    g = case.graph()
    adj_out = [[] for _ in range(V)]
    for k in np.arange(g["edges"].size):
        adj_out[int(g["edges"][k]["v1"])].append(k)
    # sortAdjOut (:48) has run in the first half: target order, stable for the short lists of these cases
    adj_out = [sorted(l, key=lambda k: int(g["edges"][k]["v2"])) for l in adj_out]
    adj_in = [[int(x) for x in g["in_nodes"][int(a):int(b)]] for a, b in zip(g["in_off"][:-1], g["in_off"][1:])]
    branching = [(int(m["v1"]), int(m["v2"])) for m in case.missing()]  # :83-85
    evidence_per_edge = {k: list(v) for k, v in case.evidence.items()}

    def edge_info(v, w):  # getEdgeInfo(v, w, false)
        for k in adj_out[v]:
            if int(g["edges"][k]["v2"]) == w:
                return case.read_len[int(g["edges"][k]["read1"])], case.read_len[int(g["edges"][k]["read2"])], int(g["edges"][k]["len0"])
        raise Ends("Edge not found")

    # :753-781
    visited_in, visited_out, in_map, out_map, in_dist, out_dist, false_in, false_out = {}, {}, {}, {}, {}, {}, set(), set()
    for node, side, dist, is_false, final in case.branches:
        if not final:
            continue
        if side == IN:
            visited_in[node], in_map[node], in_dist[node] = False, list(final), dist
            false_in |= {node} if is_false else set()
        else:
            visited_out[node], out_map[node], out_dist[node] = False, list(final), dist
            false_out |= {node} if is_false else set()
    edges_to_remove, components = [], []

    def extend_out(component, neighbors, flag):  # :941-977
        result, extended = None, False
        for node in neighbors:
            if node not in visited_out or visited_out[node]:
                continue
            if node in false_out:
                flag[0] = True
            branch = out_map[node]
            result, extended = (out_dist[node], node), True
            component += [(node, x) for x in branch]
            visited_out[node] = True
            extend_in(component, branch, flag)
        return result if extended else (0, neighbors[0])

    def extend_in(component, neighbors, flag):  # :979-1007
        for node in neighbors:
            if node not in visited_in or visited_in[node]:
                continue
            if node in false_in:
                flag[0] = True
            branch = in_map[node]
            component += [(x, node) for x in branch]
            visited_in[node] = True
            extend_out(component, branch, flag)

    for node in order(list(in_map)):  # :784-863
        if visited_in[node]:
            continue
        neighbors = in_map[node]
        flag = [node in false_in]
        comp = [(x, node) for x in neighbors]
        visited_in[node] = True
        dist1 = in_dist[node]
        dist2, outnode = extend_out(comp, neighbors, flag)
        len1, len2, olen = edge_info(outnode, node)
        if olen < 100:
            dist1, dist2 = max(dist1, len2 - olen + 100), max(dist2, len1 - olen + 100)
        else:
            dist1, dist2 = max(dist1, len2), max(dist2, len1)
        dist = dist1 + dist2 - len1 - len2 + olen
        comp = sorted(set(comp))
        if flag[0]:
            edges_to_remove += comp
        else:
            components.append((dist, comp))
    for node in order(list(out_map)):  # :882-937
        if visited_out[node]:
            continue
        neighbors = out_map[node]
        comp = [(node, x) for x in neighbors]
        dist1 = out_dist[node]
        len1, len2, olen = edge_info(node, neighbors[0])
        if olen < 100:
            dist1, dist2 = max(dist1, len1 - olen + 100), len2 - olen + 100
        else:
            dist1, dist2 = max(dist1, len1), len2
        dist = dist1 + dist2 - len1 - len2 + olen
        if node in false_out:
            edges_to_remove += comp
        else:
            components.append((dist, comp))
        visited_out[node] = True

    def count_unique_evidence(component, min_evidence):  # :1009-1272
        status, unique = [], {}
        for pair in component:
            if pair in evidence_per_edge:
                status.append(1 if evidence_per_edge[pair] else 0)
            unique.setdefault(pair, [])
        typical = len(component) in (3, 4) and len({p[1] for p in component}) == 2 and len({p[0] for p in component}) == 2
        if not status:
            raise Ends("max_element of an empty vector")
        n = len(status)

        def lst(idx):
            if component[idx] not in evidence_per_edge:
                raise Ends("at() of a missing key")
            if not evidence_per_edge[component[idx]]:
                raise Ends("front() of an empty list")
            return evidence_per_edge[component[idx]]

        while max(status) == 1:
            current = sorted(lst(i)[0] for i in range(n) if status[i] == 1)
            current_min = current[0]
            unique_min = len(current) == 1 or current_min < current[1]
            for i in range(n):
                if status[i] == 1:
                    ev = lst(i)
                    if ev[0] == current_min:
                        if unique_min:
                            unique[component[i]].append(current_min)
                        last = len(ev) == 1
                        ev.pop(0)
                        if last:
                            status[i] = 0
        keys = order(list(unique))
        count = {k: len(set(unique[k])) for k in keys}
        if case.diploid and typical:
            pairs = sorted(((k, len(unique[k])) for k in keys), key=lambda p: p[1])  # (an insertion sort of at most four: stable)
            supported, unsupported, max_count, max_edge = [], [], 0, None
            for k, _ in pairs:
                if count[k] > max_count:
                    max_count, max_edge = count[k], k
                (supported if count[k] > 0 else unsupported).append(k)
            keep = len(supported) > 0
            conflicts = lambda p: p[0] == max_edge[0] or p[1] == max_edge[1]
            if len(supported) == 1:
                return keep, [p for p in unsupported if conflicts(p)]
            if len(supported) == 2 and supported[0][0] != supported[1][0] and supported[0][1] != supported[1][1]:
                return keep, list(unsupported)
            if len(supported) == 2:
                rm, keep_complement = [], False
                if pairs[0][1] - pairs[1][1] > 0.5 * min_evidence:
                    rm.append(supported[1])
                    keep_complement = True
                return keep, rm + [p for p in unsupported if not keep_complement or conflicts(p)]
            if len(supported) > 2:
                load1 = load2 = 0
                for i, p in enumerate(supported):
                    if p != max_edge and conflicts(p):
                        load2 += pairs[i][1]
                    else:
                        load1 += pairs[i][1]
                if load1 >= load2:
                    return keep, [p for l in (unsupported, supported) for p in l if p != max_edge and conflicts(p)]
                return keep, [p for l in (unsupported, supported) for p in l if p == max_edge or (p[0] != max_edge[0] and p[1] != max_edge[1])]
        rm = [k for k in keys if count[k] < min_evidence]
        return len(rm) < len(keys), rm

    # :93-127
    node_comps = {}
    for idx, (_, comp) in enumerate(components):
        for u, v in comp:
            node_comps.setdefault(u, set()).add(idx), node_comps.setdefault(v, set()).add(idx)
    kept, outcomes, uniques = set(), [], []
    for idx, (dist, comp) in enumerate(components):  # :163-204
        neighbors = sorted(set().union(*[node_comps[u] | node_comps[v] for u, v in comp])) if case.careful else []
        skip = False
        for other in neighbors:
            if other != idx and other in kept:
                edges_to_remove += comp
                skip = True
        if skip:
            outcomes.append(BR.RED_CAREFUL)
        elif dist in case.thresholds:
            keep, rm = count_unique_evidence(comp, case.thresholds[dist])
            edges_to_remove += rm
            if keep:
                kept.add(idx)
            outcomes.append(BR.RED_KEPT if keep else BR.RED_NOT_KEPT)
        else:
            edges_to_remove += comp
            outcomes.append(BR.RED_NO_THRESHOLD)
    removed = sorted(set(edges_to_remove))  # :206-207
    for u, v in removed:  # :217-225 with OverlapGraph::removeEdge
        k = next((k for k in adj_out[u] if int(g["edges"][k]["v2"]) == v), None)
        if k is None:
            raise Ends("edge not found")
        adj_out[u].remove(k)
        if u in adj_in[v]:
            adj_in[v].remove(u)
        branching.append((u, v))
    return dict(components=[(d, [tuple(p) for p in c]) for d, c in components], outcomes=outcomes, removed=removed,
                adj_out=[[(int(g["edges"][k]["v2"]), int(g["edges"][k]["pos2"])) for k in l] for l in adj_out], adj_in=adj_in, branching=branching)


def as_expected(red, graph, branching):
    """a BranchReduction, the reduced graph and the appended records in restate()'s shape"""
    comps = [(int(c["dist"]), [tuple(int(x) for x in p) for p in red.component_edges(i)]) for i, c in enumerate(red.components)]
    V = graph["out_off"].size - 1
    adj_out = [[(int(e["v2"]), int(e["pos2"])) for e in graph["edges"][int(graph["out_off"][v]):int(graph["out_off"][v + 1])]] for v in range(V)]
    adj_in = [[int(x) for x in graph["in_nodes"][int(graph["in_off"][v]):int(graph["in_off"][v + 1])]] for v in range(V)]
    return dict(components=comps, outcomes=[int(c["outcome"]) for c in red.components], removed=[tuple(int(x) for x in p) for p in red.removed],
                adj_out=adj_out, adj_in=adj_in, branching=[(int(e["v1"]), int(e["v2"])) for e in branching])


def host_run(case):
    from haploconduct_amd import host

    return host.br_reduce(case.graph(), case.reads(), case.tables(), case.settings())


def assert_same(a, b):
    """two (BranchReduction, graph, branching) triples, table by table and byte by byte"""
    (ra, ga, ba), (rb, gb, bb) = a, b
    for k in ("components", "comp_edge", "comp_unique", "removed"):
        assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), k
    for k in ("edges", "out_off", "in_nodes", "in_off"):
        assert ga[k].tobytes() == gb[k].tobytes(), k
    assert ba.tobytes() == bb.tobytes(), "branching_edges"
    ca, cb = dict(ra.counts), dict(rb.counts)
    for k in ("ms_device", "ms_host_walk", "ms_copy", "ms_sort", "ms_edit"):
        ca.pop(k), cb.pop(k)
    assert ca == cb


WANT_KEYS = ("components", "removed", "adj_out", "adj_in", "branching")  # the recorded results of a golden case, in the file's order


def golden():
    data = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "branch_reduce.json")))

    def case(name, inputs):
        if isinstance(inputs, list):  # a plain double branch: its tables are double_branch's
            n, counts, dip = inputs
            return double_branch(name, counts, n, diploid=dip)
        return Case.from_json(inputs)

    return [(case(c[0], c[1]), dict(zip(WANT_KEYS, c[2:7])), c[7]) for c in data["cases"]], data


def recorded_order(orders):
    """order() for restate from a case's recorded iteration orders: the maps are told apart by their key sets"""
    table = {frozenset(map(_key, o)): [_key(k) for k in o] for o in orders}

    def order(keys):
        return list(table[frozenset(keys)])

    return order


def _key(k):
    return tuple(k) if isinstance(k, (list, tuple)) else k


# ---- the cases of the golden file --------------------------------------------------------------------------------------------------------

def double_branch(name, counts, n_edges=4, **kw):
    """out-nodes 0, 1 and in-nodes 2, 3 joined by 0 -> 2, 0 -> 3, 1 -> 2 and (n_edges == 4) 1 -> 3, with the given unique counts"""
    edges = [(0, 2), (0, 3), (1, 2), (1, 3)][:n_edges]
    return build(name, 4, edges, counts=dict(zip(edges, counts)), **kw)


def golden_cases():
    import itertools

    cases = [build("lone_out", 3, [(0, 1), (0, 2)], counts={(0, 1): 4, (0, 2): 1}), build("lone_in", 3, [(0, 2), (1, 2)], counts={(0, 2): 0, (1, 2): 2}),
             build("lone_out_none_kept", 3, [(0, 1), (0, 2)], counts={(0, 1): 1, (0, 2): 0}, n_missing=2)]
    # the double branch with 3 and with 4 edges, every pattern of the counts over {0, 2, 5} (min_evidence 2; ties of every shape), and a
    # near-tie for :1164
    for n in (3, 4):
        for counts in itertools.product((0, 2, 5), repeat=n):
            for dip in (1, 0):
                if dip or list(counts) == sorted(counts):  # (the general rule does not look at which edge has which count)
                    cases.append(double_branch(f"double{n}_{''.join(map(str, counts))}_{'dip' if dip else 'gen'}", counts, n, diploid=dip))
                    cases[-1].spec = [n, list(counts), dip]
    cases += [double_branch("double4_conflict_far", (9, 1, 0, 0), thresholds={d: 4 for d in range(100, 400)}),
              double_branch("double4_conflict_near", (3, 2, 0, 0), thresholds={d: 4 for d in range(100, 400)}),
              double_branch("double4_shared_ids", (3, 3, 3, 3), shared=[(0, [(0, 2), (0, 3)]), (1, [(0, 2), (1, 2), (1, 3)]), (2, [(0, 2), (0, 3), (1, 2), (1, 3)])])]
    # a false branch inside a component and alone
    cases += [double_branch("false_inside", (5, 5, 5, 5), false={(2, IN)}, n_missing=1), build("false_alone", 3, [(0, 1), (0, 2)], false={(0, OUT)}, n_missing=1),
              build("false_in_alone", 3, [(0, 2), (1, 2)], false={(2, IN)})]
    # dist without a threshold entry; overlap_len 99 / 100 at :818
    cases += [build("no_threshold", 3, [(0, 1), (0, 2)], thresholds={50: 1}), build("olen99", 3, [(0, 1, 99), (0, 2, 99)], thresholds={201: 1, 200: 9}),
              build("olen100", 3, [(0, 1, 100), (0, 2, 100)], thresholds={300: 1, 100: 9, 200: 9}),
              build("olen99_in", 3, [(0, 2, 99), (1, 2, 99)], read_len=[150, 160, 170], thresholds={d: 1 for d in range(100, 400)}),
              build("olen100_in", 3, [(0, 2, 100), (1, 2, 100)], read_len=[150, 160, 170], dist=400, thresholds={d: 1 for d in range(100, 700)})]
    # two components that share vertex 1 (0 -> {1, 2} and 1 -> {3, 4}), careful on and off, the earlier kept and the earlier not kept
    for careful in (0, 1):
        for first, second in ((3, 3), (0, 3), (3, 0)):
            cases.append(build(f"shared_vertex_c{careful}_{first}{second}", 5, [(0, 1), (0, 2), (1, 3), (1, 4)],
                               counts={(0, 1): first, (0, 2): first, (1, 3): second, (1, 4): second}, careful=careful, diploid=0))
    # asymmetric final_branch lists: the in-branch 3 lost neighbour 0, the out-branch 0 still lists 3; and a cleared branch
    cases += [double_branch("asymmetric_in", (3, 3, 3, 3), drop={(3, IN, 0)}), double_branch("asymmetric_out", (3, 0, 3, 3), drop={(1, OUT, 2)}, diploid=0),
              double_branch("cleared", (3, 3, 3, 3), cleared={(2, IN)}), double_branch("repeated_pair", (0, 3, 3, 0), diploid=0)]
    cases[-1].edges.insert(1, (0, 2, 119))  # 0 -> 2 twice: the first in target order leaves, its twin stays
    cases[-1].in_lists = {2: [1, 0, 0], 3: [1, 0]}
    cases.append(hash_case())
    return cases


def hash_case():
    """37 in-branches, so that branch_in_map rehashes twice (13 -> 29 -> 59 buckets in libstdc++).  In-branch nodes are 0 .. 35 and 62; 62
    lands in the bucket of 3, so the map's first entry is 35: neither the smallest nor the largest id.  Nodes 5 and 9 are the two in-branches
    of ONE component (sources 36 and 37 lead to both); their dists 150 and 260 lie on either side of the step of the threshold table at 150:
    started from 9 — libstdc++'s order — the component's dist is 180 and min_evidence 6 removes all four edges, started from 5 — ascending
    order — it is 120 and min_evidence 2 keeps them."""
    in_nodes = list(range(36)) + [62]
    edges, nxt = [], 63
    sources = [v for v in range(38, 62)]
    for n in in_nodes:
        if n in (5, 9):
            edges += [(36, n), (37, n)]
            continue
        pair = []
        for _ in range(2):
            if sources:
                pair.append(sources.pop(0))
            else:
                pair.append(nxt)
                nxt += 1
        edges += [(p, n) for p in pair]
    edges.sort()
    th = {d: (2 if d <= 150 else 6) for d in range(100, 400)}
    return build("rehash", nxt, edges, counts={e: 4 for e in edges}, dist={(5, IN): 150, (9, IN): 260}, thresholds=th, diploid=0)


# ---- cases that go through hc_br_evidence (the device tests) --------------------------------------------------------------------------------

def evidence_fans(seed, fans, original_readcount=None, len0=None, name="fans"):
    """A tests/_branch_evidence.Case of out-branch fans whose evidence lists have EXACTLY the sizes asked for.  Fan f: node1 with k = len(sizes)
    neighbours that share one sequence (of seed `common`, default: the fan's own) but for one position each (neighbour 0 is the sequence itself),
    so the diff list is those positions.  Neighbour j gets sizes[j] originals that are whole copies of it — each is evidence for edge
    (node1, j) and for no other —, `paired` of them as /2 mates whose /1 mate is in node1's dict (their evidence id is original_readcount +
    the /1 mate's id, :318).  shared: [(m, [j, ...])] one more original per entry, five bases around the position where neighbour m
    differs, cut from the common sequence: it agrees with every neighbour but m and is listed for the neighbours j (m not among them).  With
    `same_as` = an earlier fan's index the entry re-uses that fan's shared originals by position in the list: one id in two components.
    Returns (case, graph, sizes per fan) — graph with len0 set (default 10, the real overlap)."""
    from tests import _branch_evidence as E

    rng = np.random.default_rng(seed)
    commons = {}
    seqs, fwd, edges, dicts, singles, pairs = [], [], [], [], [], []  # pairs: (mate1 sequence, mate2 sequence)
    shared_ids = []
    pending = []  # (vertex, kind, index, index1): ids are known once the singles are counted
    for fi, f in enumerate(fans):
        sizes, L = f["sizes"], f.get("L", 40)
        k = len(sizes)
        cs = f.get("common", ("own", fi))
        if cs not in commons:
            commons[cs] = E.random_seq(rng, L)
        common = commons[cs]
        pos = [None] + [(8 + 6 * j if k <= 5 else 10 + j) for j in range(1, k)]  # (up to five neighbours: far enough apart for `shared`)
        assert pos[-1] <= L - 3
        node1 = len(seqs)
        seqs.append(E.random_seq(rng, 30) + common[:10]), fwd.append(1), dicts.append([])
        fan_shared = []
        for j in range(k):
            s = common if j == 0 else E.mutate(common, [pos[j]])
            v = len(seqs)
            seqs.append(s), fwd.append(1), dicts.append([])
            edges.append((node1, v, 30))
            n_paired = min(f.get("paired", 0), sizes[j])
            for i in range(sizes[j]):
                if i < n_paired:
                    pairs.append(("ACGT", s))
                    pending += [(v, "m2", len(pairs) - 1, 0), (node1, "m1", len(pairs) - 1, 0)]
                else:
                    singles.append(s)
                    pending += [(v, "s", len(singles) - 1, 0), (node1, "s", len(singles) - 1, 0)]
        for si, (m, js) in enumerate(f.get("shared", [])):
            assert m not in js and m > 0
            if "same_as" in f:
                sid = shared_ids[f["same_as"]][si]
            else:
                singles.append(common[pos[m] - 2:pos[m] + 3])
                sid = len(singles) - 1
            fan_shared.append(sid)
            pending += [(node1 + 1 + j, "s", sid, pos[m] - 2) for j in js] + [(node1, "s", sid, 0)]
        shared_ids.append(fan_shared)
    se, pe = len(singles), len(pairs)
    ids = {"s": lambda i: i, "m1": lambda i: se + i, "m2": lambda i: se + pe + i}
    for v, kind, i, index1 in pending:
        dicts[v].append((ids[kind](i), index1, 1))
    originals = singles + [p[0] for p in pairs] + [p[1] for p in pairs]
    orc = original_readcount if original_readcount is not None else max(len(originals), 1)
    case = E.Case(name, seqs, list(range(len(seqs))), fwd, edges, [sorted(set(d)) for d in dicts], originals, se, pe, orc)
    g = case.graph()
    g["edges"]["len0"] = 10 if len0 is None else len0
    g["edges"]["pos2"] = np.arange(g["edges"].size)
    return case, g
