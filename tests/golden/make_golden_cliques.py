#!/usr/bin/env python3
"""Generates tests/golden/cliques.json with the reference's own clique enumerator: quick-cliques, which ships inside the reference
tree and which the pipeline runs on graph.txt (src/ViralQuasispecies.cpp:397-410, `qc --algorithm=degeneracy`).

Runs only in the build container (needs /root/reference).  The UNMODIFIED quick-cliques sources are compiled into a temporary
directory with the defines of its makefile (-DPRINT_CLIQUES_ONE_BY_ONE -DALLOW_ALLOC_ZERO_BYTES, g++ -O2 -std=c++0x); nothing of them
is stored.  For every graph the script writes graph.txt, runs qc on it and stores the input — n_vertices, inclusions, the edge records
as [v1, v2] in insertion order; for the graphs built here packed (pack_pairs, pack_lines) — with qc's stdout lines as they are
(the two text lines included: the reference's clique_count counts them, src/SRBuilder.cpp:1057).  A graph.txt in which a pair stands on several lines (writeGraphToFile writes one per record) is not
something qc enumerates cliques of: it takes every line into its adjacency lists, and what it prints is no longer a set of maximal
cliques, or it dies.  For such a file qc_stdout is qc's output on the file with every line once (the pair set, which is what
hc_graph_cliques enumerates), and what qc did with the file as written is stored beside it (qc_stdout_as_written, or its exit
status).  The graphs: every graph.txt of tests/golden/graph_files.json (the reference writer's own bytes), and graphs built here
whose graph.txt is written by write_graph_txt below in the writer's format.

The script asserts from qc's output alone that no clique repeats and that every size class it set out to cover is there.

With an argument: also times qc (wall clock of the process, the file already written) on an interval graph of 100 000 vertices at
mean degree about 50 and writes the seconds to that file (not stored in the golden file).
"""
import base64
import json
import os
import random
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
QC = "/root/reference/quick-cliques"
SOURCES = ["CliqueTools", "MemoryManager", "Algorithm", "TomitaAlgorithm", "AdjacencyListAlgorithm", "HybridAlgorithm", "DegeneracyAlgorithm",
           "DegeneracyTools", "Tools", "main"]


def build_qc(tmp):
    exe = os.path.join(tmp, "qc")
    subprocess.run(["g++", "-O2", "-std=c++0x", "-w", "-DPRINT_CLIQUES_ONE_BY_ONE", "-DALLOW_ALLOC_ZERO_BYTES",
                    *[os.path.join(QC, "src", s + ".cpp") for s in SOURCES], "-o", exe], check=True)
    return exe


def write_graph_txt(V, edges, inclusions):
    """writeGraphToFile's format for a graph without reverse records or repeats: V, twice the pairs, "i,j" and "j,i" per pair."""
    lines = [f"{i},{j}\n{j},{i}\n" for i, j in edges if not inclusions[i] and not inclusions[j]]
    return f"{V}\n{2 * len(lines)}\n" + "".join(lines)


def run_qc(exe, tmp, text):
    path = os.path.join(tmp, "graph.txt")
    with open(path, "w") as f:
        f.write(text)
    t0 = time.perf_counter()
    r = subprocess.run([exe, "--algorithm=degeneracy", f"--input-file={path}"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    if r.returncode != 0:
        return None, r.returncode
    out = r.stdout
    return out.split("\n")[:-1] if out.endswith("\n") else out.split("\n"), time.perf_counter() - t0


def each_line_once(text):
    """graph.txt with every "i,j" line once (the first of its copies), the header's count corrected."""
    lines = text.split("\n")[:-1]
    body = list(dict.fromkeys(lines[2:]))
    return "\n".join([lines[0], str(len(body))] + body) + "\n"


def cliques_of(lines):
    out = []
    for ln in lines:
        tok = ln.split()
        if tok and all(t.isdigit() for t in tok):
            out.append(tuple(sorted(int(t) for t in tok)))
    return out


# ---- the graphs built here ---------------------------------------------------------------------------------------------------

def oriented(pairs):
    """Each pair once, in ascending order, as i -> j where i + j is odd and j -> i otherwise: the enumerated graph does not depend on it."""
    return [(a, b) if (a + b) & 1 else (b, a) for a, b in sorted(pairs)]


def pack_pairs(V, pairs):
    """The pairs (i < j, ascending) as base64(zlib(uint16: per vertex the number of larger neighbours, then per pair j minus the entry
    before it in i's list, the first minus i)): what a graph built here costs the golden file."""
    assert V < 65536 and pairs == sorted(set(pairs)) and all(a < b for a, b in pairs)
    counts, deltas, last = [0] * V, [], {}
    for a, b in pairs:
        counts[a] += 1
        deltas.append(b - last.get(a, a))
        last[a] = b
    return base64.b64encode(zlib.compress(struct.pack(f"<{V + len(deltas)}H", *counts, *deltas), 9)).decode()


def unpack_pairs(V, text):
    raw = zlib.decompress(base64.b64decode(text))
    vals = struct.unpack(f"<{len(raw) // 2}H", raw)
    pairs, k = [], V
    for a in range(V):
        b = a
        for _ in range(vals[a]):
            b += vals[k]
            k += 1
            pairs.append((a, b))
    return pairs


def pack_lines(lines):
    return base64.b64encode(zlib.compress("\n".join(lines).encode(), 9)).decode()


def moon_moser(parts, size):
    return [(a, b) for a in range(parts * size) for b in range(a + 1, parts * size) if a // size != b // size]


def complete(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def hub(n_triangles):
    """Vertex 0 with n_triangles pendant triangles {0, 2k + 1, 2k + 2}."""
    return [p for k in range(n_triangles) for p in ((0, 2 * k + 1), (0, 2 * k + 2), (2 * k + 1, 2 * k + 2))]


def interval(n, spread, reach, knock_out, rng):
    pos = sorted(rng.randrange(n * spread) for _ in range(n))
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            if pos[j] - pos[i] >= reach:
                break
            if rng.random() >= knock_out:
                pairs.append((i, j))
    return pairs


def gnp(n, p, rng):
    return [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < p]


def built_cases(count_cliques):
    """count_cliques(V, pairs): qc's clique count, for the G(40, 1/2) graphs, which are drawn again until they hold 400 to 520 cliques."""
    rng = random.Random(20)
    yield "moon_moser_5x3", 17, moon_moser(5, 3), rng
    for n in (63, 64, 65, 129):
        yield f"k{n}", n + 1, complete(n), rng
    yield "hub_65_triangles", 131, hub(65), rng
    yield "interval_300", 300, interval(300, 10, 60, 0.02, rng), rng
    yield "interval_2000", 2000, interval(2000, 10, 70, 0.02, rng), rng
    for k in range(3):
        pairs = gnp(40, 0.5, rng)
        while not 400 <= count_cliques(40, pairs) <= 520:
            pairs = gnp(40, 0.5, rng)
        yield f"gnp_40_{k}", 40, pairs, rng


# (cliques, largest clique) of the random graphs: what the seeds give, held here and in tests/test_cliques_host.py
PINNED = {"interval_300": (226, 13), "interval_2000": (1542, 15), "gnp_40_0": (418, 7), "gnp_40_1": (427, 6), "gnp_40_2": (460, 6)}


def main():
    with open(os.path.join(ROOT, "tests", "golden", "graph_files.json")) as f:
        files = json.load(f)["cases"]
    cases, sizes_seen = [], set()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_qc(tmp)

        def add(name, V, incl, edges, text, pairs=None):
            once = each_line_once(text)
            extra = {}
            if once != text:  # a pair on several records: qc takes every line into its adjacency lists and no longer enumerates cliques
                raw, rc = run_qc(exe, tmp, text)
                extra = dict(repeated_lines=True, qc_stdout_as_written=raw, qc_exit_as_written=0 if raw is not None else rc)
                print(f"{name}: repeated lines; qc on the file as written: " + (f"{len(cliques_of(raw))} sets" if raw is not None else f"exit {rc}"))
            lines, _ = run_qc(exe, tmp, once)
            assert lines is not None, name
            cl = cliques_of(lines)
            assert len(set(cl)) == len(cl), (name, "a clique repeats")
            assert all(len(set(c)) == len(c) and c[-1] < V for c in cl), name
            sizes_seen.update(len(c) for c in cl)
            if pairs is None:
                cases.append(dict(name=name, n_vertices=V, inclusions=incl, edges=[list(e) for e in edges], qc_stdout=lines, **extra))
            else:  # a graph built here: packed (tests/_cliques.py unpacks it into the same fields)
                assert unpack_pairs(V, pack_pairs(V, pairs)) == pairs and oriented(pairs) == edges and not any(incl)
                cases.append(dict(name=name, n_vertices=V, pairs_z=pack_pairs(V, pairs), qc_stdout_z=pack_lines(lines)))
            print(f"{name}: V={V} records={len(edges)} cliques={len(cl)} entries={sum(map(len, cl))} largest={max(map(len, cl), default=0)} "
                  f"text lines={len(lines) - len(cl)}")
            return cl

        for c in files:
            add("file_" + c["name"], c["V"], c["inclusions"], [(e[0], e[1]) for e in c["edges_in"]], c["expected"]["graph_txt"])
        for name, V, pairs, rng in built_cases(lambda V, pairs: len(cliques_of(run_qc(exe, tmp, write_graph_txt(V, oriented(pairs), [0] * V))[0]))):
            pairs = sorted(pairs)
            edges = oriented(pairs)
            cl = add(name, V, [0] * V, edges, write_graph_txt(V, edges, [0] * V), pairs)
            if name == "moon_moser_5x3":
                assert len(cl) == 245 and sum(map(len, cl)) == 1217, name
            if name[0] == "k":
                assert sorted(map(len, cl)) == [1, int(name[1:])], name
            if name.startswith("hub"):
                assert len(cl) == 65 and all(len(c) == 3 and c[0] == 0 for c in cl), name
            if name.startswith(("interval", "gnp")):
                assert PINNED[name] == (len(cl), max(map(len, cl))), (name, len(cl), max(map(len, cl)))
        timing = None
        if len(sys.argv) > 1:
            rng = random.Random(21)
            pairs = interval(100000, 10, 250, 0.0, rng)
            lines, seconds = run_qc(exe, tmp, write_graph_txt(100000, pairs, [0] * 100000))
            timing = dict(V=100000, pairs=len(pairs), cliques=len(cliques_of(lines)), qc_seconds=seconds)
            print("timing", timing)
    assert {1, 2, 3, 5, 6, 7, 13, 15, 63, 64, 65, 129} <= sizes_seen, sorted(sizes_seen)
    doc = dict(note="quick-cliques (`qc --algorithm=degeneracy`, the reference's makefile defines) on graph.txt texts: the files of "
                    "graph_files.json (file_*) and graphs built by make_golden_cliques.py.  edges = [v1, v2] per out-record in insertion order; a "
                    "graph built by the script is "
                    "packed instead: pairs_z = base64(zlib(uint16 LE: per vertex the number of larger neighbours, then per pair the step "
                    "from the entry before it in that vertex's list, the first from the vertex itself)), each pair i < j one record, i -> j "
                    "where i + j is odd, else j -> i, in ascending pair order, no inclusions; qc_stdout_z = base64(zlib(the lines joined "
                    "by newlines)).  "
                    "qc_stdout = the lines qc printed, a clique per line of integers plus its text lines; for a file with repeated lines "
                    "(repeated_lines) it is qc on the file with every line once, and qc_stdout_as_written / qc_exit_as_written is what qc "
                    "did with the file itself.", cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "cliques.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
    if timing:
        with open(sys.argv[1], "w") as f:
            json.dump(timing, f)


if __name__ == "__main__":
    main()
