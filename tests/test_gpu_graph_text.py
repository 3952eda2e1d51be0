"""graph.txt, digraph.txt and the GFA files from the device graph (hc_graph_write_text / hc_graph_text_fetch) against the reference's
own three writers (tests/golden/graph_files.json) and against the host mirror on seeded graphs at the sizes where the kernels change
path: lists of 1 / 63 / 64 / 65 / 200 records and a 4 500-record hub (the lane / wave split of the checkEdge scan and its early exit),
lists that are not in target order, repeated pairs, ids at every digit boundary up to seven digits, reads whose S lines start at every
residue mod 16; after the cleaning calls, in pieces, the refusals and the reference's asserts.

Not reachable here: ten-digit vertex ids (a graph of 10^9 vertices; std::to_string covers them on the mirror by construction, the
device's digits by the same loop that writes seven) and HC_GRAPH_TEXT_EMPTY_SEQ on the device (hc_set_reads refuses an empty sequence,
so no kept raw array holds one; the mirror's is tested in tests/test_graph_text_host.py)."""
import ctypes as C

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd.readstore import ReadSet
from haploconduct_amd.records import FLAG_IGNORE_INCLUSIONS, FLAG_RESOLVE_ORIENTATIONS
from tests import _graph_text as GT
from tests import _trans
from tests.test_gpu_graph import _admitted

pytestmark = pytest.mark.gpu

CASES = GT.load_cases()
ST = dict(edge_threshold=0.9, merge_contigs=0.05)


@pytest.fixture(scope="module")
def scorer():
    if hc.device_count() < 1:
        pytest.fail("no HIP device")
    with hc.EdgeScorer(hc.Settings()) as sc:
        sc.sr_keep_device(True)
        yield sc


def read_set(bases, off, first):
    return ReadSet(bases, np.full(bases.size, ord("I"), np.uint8), off, first, np.arange(first.size - 1))


def both(sc, graph, kind, raw=None, **st):
    """(device text, device counts, mirror text, mirror counts) of a loaded graph."""
    reads = dict(zip(("bases", "seq_off", "read_first_seq"), raw)) if raw is not None else {}
    want, wc = GT.mirror(graph).write_text(kind, **reads, **st)
    got, gc = sc.graph_write_text(kind, **st)
    return got, gc, want, wc


def same_counts(gc, wc):
    return all(gc[k] == wc[k] for k in gc if k != "ms_device")


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_device_equals_reference(scorer, name):
    case = next(c for c in CASES if c["name"] == name)
    scorer.set_reads(read_set(*GT.raw_reads(case["reads"])))
    scorer.graph_load(*GT.case_graph(case))
    for kind in GT.KINDS:
        text, counts = scorer.graph_write_text(kind, **GT.settings_of(case))
        assert text == case["expected"][GT.EXPECTED[kind]].encode(), (name, kind)
        GT.check_counts(counts, case, kind, text, (name, kind))
        assert counts["ms_device"] > 0


def lists_graph():
    """Out-lists of 1, 63, 64, 65 and 200 records and a 4 500-record hub, all shuffled (no list is in target order), with reverse records
    that make the checkEdge scan walk each of them: to the first, a middle and the last list position, and for a pair that is absent."""
    rng = np.random.default_rng(21)
    V = 7000
    v1, v2 = [], []
    hub = 10
    targets = rng.permutation(np.arange(100, 6000))[:4500]  # the hub's list in list order
    v1 += [hub] * 4500
    v2 += targets.tolist()
    back = {int(targets[0]), int(targets[2250]), int(targets[4499])} | set(int(t) for t in targets[rng.random(4500) < 0.2])
    absent = [int(x) for x in np.setdiff1d(np.arange(100, 6000), targets)[:40]]
    for t in sorted(back) + absent:
        v1.append(t)
        v2.append(hub)
    for src, deg in ((20, 1), (21, 63), (22, 64), (23, 65), (24, 200)):
        tg = rng.permutation(np.arange(6000, 6900))[:deg]
        v1 += [src] * deg
        v2 += tg.tolist()
        for t in {int(tg[0]), int(tg[deg // 2]), int(tg[-1])}:
            v1.append(t)
            v2.append(src)
        v1.append(6950 + src - 20)  # a reverse record without its forward one
        v2.append(src)
    p = rng.permutation(len(v1))
    recs = GT.records_for(np.array(v1)[p], np.array(v2)[p], 5)
    incl = np.zeros(V, np.uint8)
    incl[[6990, 6991, int(targets[7])]] = 1  # no out-edges: 6990, 6991; a target of the hub that has none either
    keep = ~np.isin(recs["v1"], np.flatnonzero(incl))
    return (*_trans.csr_from_inserts(recs[keep], V), incl)


def repeated_graph():
    """An interval graph with every edge's reverse record and repeated pairs in both directions, inserted in random order: first copies
    with a score of 0.0, -1 and above 0 decide; long lists with repeats."""
    rng = np.random.default_rng(22)
    V = 1500
    a, b = _trans.interval_edges(V, 6, seed=7)
    rev = rng.random(len(a)) < 0.6
    rep = rng.random(len(a)) < 0.3
    v1 = np.concatenate([a, b[rev], a[rep], b[rev & rep], b[rev & rep]])
    v2 = np.concatenate([b, a[rev], b[rep], a[rev & rep], a[rev & rep]])
    p = rng.permutation(len(v1))
    recs = GT.records_for(v1[p], v2[p], 6)
    return (*_trans.csr_from_inserts(recs, V), np.zeros(V, np.uint8))


def digits_graph():
    """V = 1 000 001: ids on both sides of every digit boundary up to seven digits, reverse pairs across them."""
    V = 1000001
    pairs = []
    for lo, hi in ((9, 10), (99, 100), (999, 1000), (99999, 100000), (999999, 1000000)):
        pairs += [(lo, hi), (hi, lo), (hi, 0), (lo, 1000000), (0, lo), (5, hi)]
    recs = GT.records_for(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), 8)
    return (*_trans.csr_from_inserts(recs, V), np.zeros(V, np.uint8))


@pytest.mark.parametrize("make", [lists_graph, repeated_graph, digits_graph], ids=["lists", "repeated", "digits"])
def test_device_equals_mirror_cliques_and_digraph(scorer, make):
    graph = make()
    scorer.graph_load(*graph)
    for kind in ("cliques", "digraph"):
        got, gc, want, wc = both(scorer, graph, kind, **ST)
        assert wc["status"] == 0 and len(want) > 0
        assert got == want, kind
        assert same_counts(gc, wc), (gc, wc)
    if make is lists_graph:
        edges, out_off = graph[0], graph[1]
        deg = np.diff(out_off.astype(np.int64))
        assert {1, 63, 64, 65, 200} <= set(deg.tolist()) and deg.max() >= 4400
        assert (np.diff(edges["v2"][int(out_off[10]):int(out_off[11])].astype(np.int64)) < 0).any(), "the hub's list is not in target order"


GFA_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 1500]


def test_gfa_equals_mirror_at_every_alignment(scorer):
    """Reads of 1, 15, 16, 17, 63, 64, 65 and 1 500 bases, forwards and reversed (--add_duplicates: V = 2 * n_reads), a few pairs behind
    the singles, links between them: the sequences of the S lines start at every residue mod 16, both ways."""
    rng = np.random.default_rng(31)
    n_singles, n_pairs = 72, 6
    n_reads = n_singles + n_pairs
    table = GT.random_reads([GFA_LENGTHS[k % 8] for k in range(n_singles)], 32)
    table += [[s[0], s[0][::-1] + "A", 1] for s in GT.random_reads([20] * n_pairs, 33)]
    raw = GT.raw_reads(table)
    V = 2 * n_reads
    v1, v2 = rng.integers(0, V, 900), rng.integers(0, V, 900)
    ok = v1 != v2
    graph = (*_trans.csr_from_inserts(GT.records_for(v1[ok], v2[ok], 9), V), np.zeros(V, np.uint8))
    scorer.set_reads(read_set(*raw))
    scorer.graph_load(*graph)
    got, gc, want, wc = both(scorer, graph, "gfa", raw, n_singles=n_singles)
    assert wc["status"] == 0 and wc["n_segments"] == 2 * n_singles and wc["l_count"] > 0 and wc["c_count"] > 0
    assert got == want
    assert same_counts(gc, wc), (gc, wc)
    # where the copied bytes land: behind "S\t<id>\t"
    starts = {False: set(), True: set()}
    at = 0
    for line in want.split(b"\n")[:-1]:
        if line[:1] == b"S":
            v = int(line.split(b"\t")[1])
            starts[v >= n_reads].add((at + 3 + len(str(v))) % 16)
        at += len(line) + 1
    assert starts[False] == set(range(16)) and starts[True] == set(range(16))
    for n in GFA_LENGTHS:
        assert sum(1 for ln in want.split(b"\n") if ln[:1] == b"S" and len(ln.split(b"\t")[2]) == n) >= 2


def test_gfa_a_million_segments_and_an_edgeless_graph(scorer):
    """V = 1 000 001 two-base reads: seven-digit ids in S and L lines; then the same reads with no edge at all."""
    V = 1000001
    rng = np.random.default_rng(41)
    bases = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, 2 * V)]
    raw = (bases, np.arange(0, 2 * V + 1, 2, dtype=np.uint64), np.arange(V + 1, dtype=np.uint32))
    scorer.set_reads(read_set(*raw))
    graph = digits_graph()
    scorer.graph_load(*graph)
    got, gc, want, wc = both(scorer, graph, "gfa", raw, n_singles=V)
    assert got == want and same_counts(gc, wc) and gc["n_segments"] == V
    assert b"\nS\t1000000\t" in got and b"\nL\t999999\t+\t1000000\t+\t" in got
    empty = (graph[0][:0], np.zeros(V + 1, np.uint64), graph[2][:0], np.zeros(V + 1, np.uint64), graph[4])
    scorer.graph_load(*empty)
    got, gc, want, wc = both(scorer, empty, "gfa", raw, n_singles=1000)
    assert got == want and gc["n_segments"] == 1000 and gc["l_count"] == gc["c_count"] == 0
    assert scorer.graph_write_text("digraph")[0] == b""
    assert scorer.graph_write_text("cliques")[0] == b"1000001\n0\n"


def test_negative_len0(scorer):
    """len0 is a signed int in the record: the device writes std::to_string(int) of what it is given (the mirror's Edge cannot hold one)."""
    recs = _trans.make_records(np.array([0, 1, 2]), np.array([1, 2, 0]), 1)
    recs["len0"] = [-2147483648, -17, 0]
    recs["perc"] = [100, 5, 100]
    graph = (*_trans.csr_from_inserts(recs, 3), None)
    scorer.set_reads(read_set(*GT.raw_reads([["ACG", "", 0], ["T", "", 0], ["GGN", "", 0]])))
    scorer.graph_load(*graph)
    text, c = scorer.graph_write_text("gfa", n_singles=3)
    assert text == (b"H\tVN:Z:1.0\nS\t0\tACG\nL\t0\t+\t1\t+\t-2147483648M\nS\t1\tT\nL\t1\t+\t2\t+\t-17M\nS\t2\tGGN\nL\t2\t+\t0\t+\t0M\n")
    assert (c["n_segments"], c["l_count"], c["c_count"], c["n_lines"]) == (3, 1, 2, 7)


def test_after_cleaning_in_pieces_and_replaced(scorer):
    """The text of the graph hc_graph_remove_transitive and hc_graph_remove_branches leave equals the mirror's on the graph the mirror
    cleaned; the call leaves the graph as it was; a 4 KiB piecewise fetch equals the whole; the next call replaces the text and a
    cleaning call drops it."""
    V = 3000
    a, b = _trans.interval_edges(V, 5, seed=12)
    edges, out_off, in_nodes, in_off, incl = _trans.shuffled_graph(a, b, V, 13)
    incl[:] = 0
    m = _trans.Mirror(edges, out_off, in_nodes, in_off, incl)
    scorer.graph_load(edges, out_off, in_nodes, in_off, incl)
    for step in ("transitive", "branches"):
        if step == "transitive":
            m.g.remove_transitive_edges(1, False)
            scorer.graph_remove_transitive(1, False)
        else:
            m.g.remove_branches()
            scorer.graph_remove_branches()
        before = scorer.graph_fetch()
        for kind in ("cliques", "digraph"):
            want, wc = m.g.write_text(kind, edge_threshold=0.0)
            got, gc = scorer.graph_write_text(kind, edge_threshold=0.0)
            assert wc["status"] == 0 and got == want and same_counts(gc, wc), (step, kind)
        after = scorer.graph_fetch()
        assert all(np.array_equal(before[k], after[k]) for k in before), step
    whole, c = scorer.graph_write_text("digraph")
    assert len(whole) > 3 * 4096
    pieces, _ = scorer.graph_write_text("digraph", piece_bytes=4096)
    assert pieces == whole
    # the text stays for further fetches; another kind replaces it
    buf = np.zeros(len(whole), np.uint8)
    N.check(N.lib.hc_graph_text_fetch(scorer._ctx, 5, 100, buf.ctypes.data), "hc_graph_text_fetch")
    assert buf[:100].tobytes() == whole[5:105]
    cliques, cc = scorer.graph_write_text("cliques", edge_threshold=0.0)
    assert cliques != whole
    big = np.zeros(cc["n_bytes"], np.uint8)
    N.check(N.lib.hc_graph_text_fetch(scorer._ctx, 0, cc["n_bytes"], big.ctypes.data), "hc_graph_text_fetch")
    assert big.tobytes() == cliques
    # a range outside the text: HC_ERR_ARG and nothing copied
    buf[:] = 7
    assert N.lib.hc_graph_text_fetch(scorer._ctx, cc["n_bytes"] - 3, 4, buf.ctypes.data) == -1
    assert N.lib.hc_graph_text_fetch(scorer._ctx, cc["n_bytes"] + 1, 0, buf.ctypes.data) == -1
    assert (buf == 7).all()
    assert N.lib.hc_graph_text_fetch(scorer._ctx, cc["n_bytes"], 0, None) == 0
    # every call that replaces or cleans the graph drops the text
    scorer.graph_remove_branches()
    assert N.lib.hc_graph_text_fetch(scorer._ctx, 0, 1, buf.ctypes.data) == -5
    scorer.graph_write_text("digraph")
    scorer.graph_load(edges, out_off, in_nodes, in_off, incl)
    assert N.lib.hc_graph_text_fetch(scorer._ctx, 0, 1, buf.ctypes.data) == -5


def test_refusals():
    st, c = N.hc_graph_text_settings(0.9, 0.0, 0), N.hc_graph_text_counts()
    buf = np.zeros(16, np.uint8)
    edges, out_off, in_nodes, in_off, incl = _trans.shuffled_graph(*_trans.interval_edges(200, 4, seed=3), 200, 4)
    with hc.EdgeScorer(hc.Settings()) as sc:
        for kind in GT.KINDS:  # no graph
            with pytest.raises(hc.HcError) as err:
                sc.graph_write_text(kind)
            assert err.value.status == -5  # HC_ERR_STATE
        assert N.lib.hc_graph_text_fetch(sc._ctx, 0, 0, buf.ctypes.data) == -5  # no text
        sc.graph_load(edges, out_off, in_nodes, in_off)
        assert N.lib.hc_graph_write_text(sc._ctx, 3, C.byref(st), C.byref(c)) == -1  # unknown kind
        assert N.lib.hc_graph_write_text(sc._ctx, 0, None, C.byref(c)) == -1
        assert N.lib.hc_graph_write_text(sc._ctx, 0, C.byref(st), None) == -1
        with pytest.raises(hc.HcError) as err:  # GFA without kept raw arrays: no store at all, then a store that was not kept
            sc.graph_write_text("gfa")
        assert err.value.status == -5
        raw = GT.raw_reads(GT.random_reads([30] * 200, 1))
        sc.set_reads(read_set(*raw))
        with pytest.raises(hc.HcError) as err:
            sc.graph_write_text("gfa", n_singles=10)
        assert err.value.status == -5
        sc.sr_keep_device(True)
        sc.set_reads(read_set(*raw))
        with pytest.raises(hc.HcError) as err:  # more singles than reads
            sc.graph_write_text("gfa", n_singles=201)
        assert err.value.status == -1
        assert N.lib.hc_graph_text_fetch(sc._ctx, 0, 0, buf.ctypes.data) == -5  # a refused call keeps no text
        # the context stays usable
        text, cc = sc.graph_write_text("gfa", n_singles=200)
        want, wc = GT.mirror((edges, out_off, in_nodes, in_off, incl * 0)).write_text("gfa", n_singles=200, bases=raw[0], seq_off=raw[1], read_first_seq=raw[2])
        assert text == want and same_counts(cc, wc)
    # a resolved graph with tied lists is refused as the cleaning calls refuse it
    V, m = 300, 40000
    reads, adm = _admitted(1, V, m, 0.0)
    with hc.EdgeScorer(hc.Settings(edge_threshold=0.97, flags=FLAG_RESOLVE_ORIENTATIONS | FLAG_IGNORE_INCLUSIONS)) as sc:
        sc.set_reads(reads)
        sgot = sc.graph_resolve(adm, V, sorted_order=True)
        assert sgot["counts"]["n_tied_lists"] > 0
        with pytest.raises(hc.HcError) as err:
            sc.graph_write_text("digraph")
        assert err.value.status == -5
        still = sc.graph_fetch()
        assert still["edges"].tobytes() == sgot["edges"].tobytes()


def _plant(V, pairs, incl=None, **fields):
    r = _trans.make_records(np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64), 1)
    r["score"], r["mismatch_rate"] = 0.99, 0.0
    for k, v in fields.items():
        r[k] = v
    return (*_trans.csr_from_inserts(r, V), np.zeros(V, np.uint8) if incl is None else np.array(incl, np.uint8))


def _check_status(sc, graph, kind, expect, raw=None, **st):
    sc.graph_load(*graph)
    got, gc, want, wc = both(sc, graph, kind, raw, **st)
    assert got == b"" and want == b""
    assert (N.GRAPH_TEXT_STATUS[gc["status"]], gc["bad_v"], gc["bad_pos"]) == expect
    assert (wc["status"], wc["bad_v"], wc["bad_pos"]) == (gc["status"], gc["bad_v"], gc["bad_pos"])
    assert gc["n_bytes"] == 0 and gc["n_lines"] == 0
    buf = np.zeros(4, np.uint8)
    assert N.lib.hc_graph_text_fetch(sc._ctx, 0, 0, buf.ctypes.data) == -5  # no text kept


def test_assert_statuses_first_in_file_order(scorer):
    """Every status the device can meet (EMPTY_SEQ: see the module's note), two or more planted each time: the first record in file
    order is reported, as by the mirror, whichever workgroup met it; and the context goes on working."""
    # self-loops at vertex 700 position 1 and, later in the file, at 700 position 3 and 5000 position 0; 6000 records in front
    a, b = _trans.interval_edges(6000, 3, seed=2)
    pairs = list(zip(a.tolist(), b.tolist())) + [(700, 5999), (700, 700), (700, 2), (700, 700), (5000, 5000)]
    own = [p for p in pairs if p[0] == 700]
    base_700 = sum(1 for p in zip(a.tolist(), b.tolist()) if p[0] == 700)
    raw = GT.raw_reads(GT.random_reads([20] * 6000, 2))
    scorer.set_reads(read_set(*raw))
    g = _plant(6000, pairs)
    assert own[base_700 + 1] == (700, 700)
    for kind in GT.KINDS:
        _check_status(scorer, g, kind, ("SELF_LOOP", 700, base_700 + 1), raw, n_singles=6000, edge_threshold=0.0)
    # inclusion vertices with out-edges: 40 and 3000; a self-loop behind the first of them
    incl = np.zeros(6000, np.uint8)
    incl[[40, 3000]] = 1
    g = _plant(6000, list(zip(a.tolist(), b.tolist())) + [(41, 41)], incl=incl)
    _check_status(scorer, g, "cliques", ("INCLUSION_HAS_EDGES", 40, 0), edge_threshold=0.0)
    # weak first copies: 90 -> 80 is looked up from 80's list (three records in front of it), and 4000 -> 3990 likewise, later
    pairs = [(80, 81), (80, 82), (80, 83), (80, 90), (80, 90), (90, 95), (90, 80), (3990, 4000), (4000, 3990)]
    score = [0.99, 0.99, 0.99, 0.5, 0.99, 0.99, 0.99, 0.2, 0.99]
    mm = [0, 0, 0, 0.3, 0, 0, 0, 0.3, 0]
    g = _plant(6000, pairs, score=score, mismatch_rate=mm)
    _check_status(scorer, g, "cliques", ("WEAK_EDGE", 90, 1), edge_threshold=0.9, merge_contigs=0.1)
    scorer.graph_load(*g)
    text, c = scorer.graph_write_text("cliques", edge_threshold=0.9, merge_contigs=0.3)  # the mismatch rate saves both
    assert c["status"] == 0 and c["n_pairs"] == 7
    # GFA: pairs among the singles (reads 50 and 51 own two sequences), bad bases in reads 30 and 10 — which only their reversed copies meet
    table = GT.random_reads([24] * 60, 3)
    table[50] = [table[50][0], "ACGT", 1]
    table[51] = [table[51][0], "ACGT", 1]
    table[30][0] = table[30][0][:5] + "X" + table[30][0][6:]
    table[10][0] = "-" + table[10][0][1:]
    raw = GT.raw_reads(table)
    scorer.set_reads(read_set(*raw))
    g = _plant(120, [(0, 1), (1, 2), (60, 61), (70, 10), (119, 3)])
    _check_status(scorer, g, "gfa", ("PAIRED_IN_SINGLES", 50, 0), raw, n_singles=60)
    _check_status(scorer, g, "gfa", ("BAD_BASE", 70, 0), raw, n_singles=50)
    _check_status(scorer, g, "gfa", ("BAD_BASE", 70, 0), raw, n_singles=31)
    scorer.graph_load(*g)
    got, gc, want, wc = both(scorer, g, "gfa", raw, n_singles=10)  # reads 10 and 30 are no segments now; forwards they would be fine
    assert gc["status"] == 0 and got == want and same_counts(gc, wc)
    g1 = _plant(60, [(0, 1), (10, 30), (30, 10)])
    scorer.graph_load(*g1)
    got, gc, want, wc = both(scorer, g1, "gfa", raw, n_singles=40)  # V = n_reads: no reversed copy exists
    assert gc["status"] == 0 and got == want and b"X" in got and b"\t-" in got
    # a long reversed read whose bad base is its very last byte (the wave's scan, last chunk)
    table = GT.random_reads([1500, 70, 64], 4)
    table[0][0] = table[0][0][:-1] + "x"
    raw = GT.raw_reads(table)
    scorer.set_reads(read_set(*raw))
    g = _plant(6, [(0, 1)])
    _check_status(scorer, g, "gfa", ("BAD_BASE", 3, 0), raw, n_singles=3)
