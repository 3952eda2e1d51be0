"""hc_fno1_from_graph on the device (include/hcsr.h).  The expected result is always hc_fno1_run on the host threads (HC_FNO=host) for the
arrays fno.input_from_context fetches from the same context — the route the golden tests pin to the reference's own output: the walk's edge
list array by array and per segment (against hc_host_fno1_walk_edges), the text byte for byte, the four counters.  A cleaned graph of
2 000 vertices under every flag; out-lists of 63 / 64 / 65 / 300 records under checkEdge and inclusion groups of 1, 2, 3, 63, 64, 65 and 300
records; the tables hc_sr_merge_next and hc_sr_clique_next keep; the lines as records and through a text block; the refusals; two calls; one
graph of 3 * 10^5 records."""
import functools

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import consensus as SR
from haploconduct_amd import fno as F
from haploconduct_amd import host
from haploconduct_amd.records import LINE_DTYPE
from tests import _clique_merge as CM
from tests import _edge_merge as EM
from tests import _fno1_resident as R
from tests import _merge_next as M
from tests import _tips
from tests import _trans

pytestmark = pytest.mark.gpu
NOT_ON_DEVICE, ERR_STATE, ERR_ARG = -11, -5, -1


# ---- 1. the whole route ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _route():
    V = 2000
    a, b = _trans.interval_edges(V, 12, seed=1)
    tables = R.seeded_tables(7, V, 300)
    tables[0]["len1"] = 250  # the reads of tip_geometry: pos1 stays below the length
    p = np.random.default_rng(2).permutation(len(a))
    recs = R.graph_records(a[p], b[p], tables[0], seed=3)
    recs, geom = _tips.tip_geometry(recs, V, V, seed=4)
    incl = (np.random.default_rng(5).random(V) < 0.02).astype(np.uint8)
    return V, recs, geom, incl, tables


def _cleaned(sc):
    V, recs, geom, incl, tables = _route()
    R.load(sc, recs, V, incl)
    sc.graph_remove_inclusions()
    sc.graph_remove_transitive(1, False)
    sc.graph_remove_tips(150, geom)
    sc.graph_remove_branches()
    return tables


@pytest.fixture(scope="module")
def route_ctx():
    with hc.EdgeScorer() as sc:
        tables = _cleaned(sc)
        edges = F.edges_from_graph(sc.graph_fetch()["edges"])
        nonedges = R.seeded_nonedges(11, 3000, tables[0], edges)
        yield sc, tables, nonedges


def test_the_cleaned_graph_has_every_source(route_ctx):
    sc, tables, nonedges = route_ctx
    assert 18000 < len(_route()[1]) < 22000
    _, goff, grecs = sc.graph_inclusion_edges()
    assert len(goff) > 10 and len(grecs) > 100 and len(sc.graph_branching_edges()) > 100 and len(sc.graph_fetch()["edges"]) > 500


@pytest.mark.parametrize("flags", [0, F.RESOLVE_ORIENTATIONS, F.NO_INCLUSIONS, F.OPTIMIZE, F.RESOLVE_ORIENTATIONS | F.NO_INCLUSIONS | F.OPTIMIZE])
def test_whole_route_under_every_flag(route_ctx, flags):
    sc, tables, nonedges = route_ctx
    inp, text, counters = R.expected(sc, tables, nonedges, flags=flags, edge_threshold=0.97)
    res = sc.fno1_from_graph(tables, nonedges, 0.97, flags)
    R.assert_same_run(sc, res, inp, text, counters, f"flags {flags}")
    c = res.counts
    assert c["n_lines"] > 1000 and c["u2sr"] and c["v2sr"] and c["sr2sr"] and c["copied"] and c["ms_device"] > 0
    assert c["n_induced_pairs"] > c["n_induced"] > 0 and c["n_branching"] > 0
    if flags & F.OPTIMIZE:
        assert c["n_nonedges_kept"] == 0
    else:
        assert 0 < c["n_nonedges_kept"] < len(nonedges) * 0.8  # a third sits behind an edge, in either direction
    if flags == F.RESOLVE_ORIENTATIONS:  # 4. the lines as records: the columns of the text, line by line
        want, _ = _parsed(text)
        lines = _lines_of(sc)[2]
        for f in LINE_DTYPE.names:
            assert np.array_equal(lines[f], want[f]), f


# ---- 2. the size classes ------------------------------------------------------------------------------------------------------------------
HUBS = {10: 63, 11: 64, 12: 65, 13: 300}
GROUPS = {20: 1, 21: 2, 22: 3, 23: 63, 24: 64, 25: 65, 26: 300}


@functools.lru_cache(maxsize=None)
def _classes():
    """Hubs with out-lists of 63 / 64 / 65 / 300 records into a small pool; inclusion vertices whose groups have 1 .. 300 records, half of
    them in-edges from the hubs and from a small pool, the others out-edges into the hubs and the hubs' targets: the induced pairs y -> x
    then ask checkEdge to scan a hub's list as v's (a hit anywhere, or none) or as w's (the reverse list)."""
    V = 2000
    rng = np.random.default_rng(21)
    pool, plain = np.arange(100, 420), np.arange(1000, 1060)
    v1, v2 = [], []
    for h, n in HUBS.items():
        t = rng.choice(np.concatenate([pool, plain]), n, replace=False)
        v1 += [h] * n
        v2 += t.tolist()
    for w, l in GROUPS.items():
        n_in = l // 2
        ins = rng.choice(np.concatenate([list(HUBS), np.arange(1000, 1200)]), n_in, replace=False) if n_in else []
        outs = rng.choice(np.concatenate([list(HUBS), pool]), l - n_in, replace=False)
        v1 += [int(y) for y in ins] + [w] * (l - n_in)
        v2 += [w] * n_in + [int(x) for x in outs]
    a, b = _trans.interval_edges(600, 3, seed=22)  # and a plain stretch of graph
    v1 += (a + 1200).tolist()
    v2 += (b + 1200).tolist()
    tables = R.seeded_tables(23, V, 150, paired_frac=0.1)
    p = rng.permutation(len(v1))
    recs = R.graph_records(np.asarray(v1)[p], np.asarray(v2)[p], tables[0], seed=24, scores=(0.0, 0.5, 1.0))
    incl = np.zeros(V, np.uint8)
    incl[list(GROUPS)] = 1
    return V, recs, incl, tables


def test_long_lists_under_check_edge_and_groups_of_every_size():
    V, recs, incl, tables = _classes()
    with hc.EdgeScorer() as sc:
        R.load(sc, recs, V, incl)
        sc.graph_remove_inclusions()
        g = sc.graph_fetch()
        deg = np.diff(g["out_off"].astype(np.int64))
        assert [int(deg[h]) for h in HUBS] == list(HUBS.values())
        gv, goff, _ = sc.graph_inclusion_edges()
        sizes = dict(zip(gv.tolist(), np.diff(goff.astype(np.int64)).tolist()))
        assert sizes == GROUPS
        edges = F.edges_from_graph(g["edges"])
        nonedges = R.seeded_nonedges(25, 2000, tables[0], edges, behind_frac=0.5)
        assert (np.isin(nonedges["v1"], list(HUBS)) | np.isin(nonedges["v2"], list(HUBS))).sum() > 200
        inp, text, counters = R.expected(sc, tables, nonedges, edge_threshold=0.9)
        res = sc.fno1_from_graph(tables, nonedges, 0.9)
        R.assert_same_run(sc, res, inp, text, counters, "size classes")
        need = sum(l * (l - 1) // 2 for l in GROUPS.values())
        assert need > 44850 and res.counts["n_induced_pairs"] == need and 0 < res.counts["n_induced"] < need
        # one pair fewer than the groups hold is refused, and nothing is changed
        with pytest.raises(hc.HcError) as e:
            sc.fno1_from_graph(tables, nonedges, 0.9, max_induced_pairs=need - 1)
        assert e.value.status == NOT_ON_DEVICE
        sc._fno1 = res
        assert sc.fno1_text() == text
        again = sc.fno1_from_graph(tables, nonedges, 0.9, max_induced_pairs=need)
        R.assert_same_run(sc, again, inp, text, counters, "max_induced_pairs = the need")


# ---- 3. kept tables, 4. lines ---------------------------------------------------------------------------------------------------------------
def _lines_of(sc):
    p, n = sc.fno1_lines_device()
    return p, n, sc.found_lines_fetch(p, n)


def _parsed(text):
    """The 13 columns of every line as LINE_DTYPE: through the product's line parser (host.parse_overlap, the tokeniser of hc_host_parse_text)
    where it takes the line; a line with a negative number is not plain for it, and is split at its tabs here, a number being the 32 bits of
    the int the text prints (include/hcsr.h).  -> (records, lines the parser took)"""
    out, plain = np.zeros(text.count(b"\n"), LINE_DTYPE), 0
    for k, ln in enumerate(text.decode().split("\n")[:-1]):
        rc, o = host.parse_overlap(ln)
        if rc == 0:
            plain += 1
            out[k] = (o["id1"], o["id2"], o["pos1"], o["pos2"], o["perc"], 0, o["len1"], o["len2"], ord(o["ord"]), ord(o["ori1"]), ord(o["ori2"]),
                      ord(o["type1"]), ord(o["type2"]), (0, 0, 0))
        else:
            c = ln.split("\t")
            assert len(c) == 13 and c[8] == "0", ln
            u = lambda x: int(x) & 0xFFFFFFFF
            out[k] = (int(c[0]), int(c[1]), u(c[2]), u(c[3]), u(c[7]), 0, u(c[9]), u(c[10]), ord(c[4]), ord(c[5]), ord(c[6]), ord(c[11]), ord(c[12]), (0, 0, 0))
    return out, plain


def _plain_rows(g):
    """seeded_graph's records as an overlaps file may hold them: no negative position, ord '-' unless both reads are paired"""
    first = g["reads"].read_first_seq.astype(np.int64)
    paired = (first[1:] - first[:-1]) == 2
    rows = [list(r) for r in g["rows"] if r[4] >= 0 and r[5] >= 0]
    for r in rows:
        if not (paired[r[2]] and paired[r[3]]):
            r[8] = ord("-")
    return rows


def _kept_against_host_tables(sc, dev, what):
    inp, text, counters = R.expected(sc, dev)
    kept = sc.fno1_from_graph(None)
    R.assert_same_run(sc, kept, inp, text, counters, what + ": kept tables")
    kept_text, kept_edges = sc.fno1_text(), sc.fno1_edges()
    _, n, kept_lines = _lines_of(sc)
    caller = sc.fno1_from_graph(dev)
    R.assert_same_run(sc, caller, inp, text, counters, what + ": host tables")
    assert sc.fno1_text() == kept_text and sc.fno1_edges()[0].tobytes() == kept_edges[0].tobytes(), what
    strip = lambda c: {k: v for k, v in c.items() if k != "ms_device"}
    assert strip(kept.counts) == strip(caller.counts), what
    assert n == kept.counts["n_lines"] > 50, what
    return text, kept_lines


def test_tables_kept_by_merge_next_and_the_lines():
    g = EM.seeded_graph(seed=6, n_reads=400, template_len=6000, long_lists=(63,))
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.graph_load(*EM.csr(g["V"], _plain_rows(g)))
        with pytest.raises(hc.HcError) as e:  # before any merge call
            sc.fno1_from_graph(None)
        assert e.value.status == ERR_STATE
        pairs = sc.graph_merge_pairs()
        edge = sc.sr_edge_merge(pairs, g["vertex_read"], g["vertex_fwd"])
        dev = sc.sr_merge_next(pairs, edge, g["vertex_read"], g["vertex_fwd"], keep_singletons=50)
        assert not dev.empty and len(dev.srs) > 50
        text, lines = _kept_against_host_tables(sc, dev, "merge_next")
        # 4. the lines as records are the parsed text, field by field
        want, plain = _parsed(text)
        assert plain == len(want) > 50, (plain, len(want))
        for f in LINE_DTYPE.names:
            assert np.array_equal(lines[f], want[f]), f
        # ... and a text block fed the records returns what one fed the text returns (the store is the new one)
        sc.set_ids(np.arange(dev.new_read_count, dtype=np.uint64))
        by_text = sc.score_text(text, block_bytes=max(len(text), 64))
        p, n = sc.fno1_lines_device()
        by_lines = sc.score_lines_device(p, n)
        assert len(by_text) == 1 and by_text[0]["n_lines"] == n
        for k in ("n_lines", "lines_read", "needs_host", "n_nonplain", "n_unknown_id", "self_overlaps", "silently_dropped", "prefilter_rejected", "scored",
                  "n_rows", "n_rejected"):
            assert by_lines[k] == by_text[0][k], (k, by_lines[k], by_text[0][k])
        assert by_text[0]["needs_host"] == 0 and by_text[0]["scored"] + by_text[0]["n_rejected"] > 0
        for k in ("rows", "rejected"):
            assert sorted(r.tobytes() for r in by_lines[k]) == sorted(r.tobytes() for r in by_text[0][k]), k
        # another vertex count, then hc_reset: the kept tables are refused
        a, b = _trans.interval_edges(300, 3, seed=9)
        R.load(sc, _trans.make_records(a, b, 9), 300)
        with pytest.raises(hc.HcError) as e:
            sc.fno1_from_graph(None)
        assert e.value.status == ERR_STATE
        sc.reset(hc.Settings())
        with pytest.raises(hc.HcError) as e:
            sc.fno1_from_graph(None)
        assert e.value.status == ERR_STATE


def test_tables_kept_by_clique_next():
    g = CM.seeded_cliques()
    cliques = [c for c in g["cliques"] if 3 <= len(c) <= 8]
    assert len(cliques) > 40 and {len(c) for c in cliques} >= {3, 5}
    off, nodes = SR.clique_csr(cliques)
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.graph_load(*EM.csr(g["V"], g["rows"]))
        merged = sc.sr_clique_merge(off, nodes, g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        dev = sc.sr_clique_next(off, nodes, merged, g["vertex_read"], g["vertex_fwd"], keep_singletons=50)
        assert not dev.empty and len(dev.srs) > 20
        _kept_against_host_tables(sc, dev, "clique_next")
        # a merge call that ends empty (no pair, no vertex) clears the kept tables all the same; so does any later successful one until it ends
        try:
            assert sc.sr_merge_next(np.zeros((0, 2), np.uint32), M.empty_edge(), np.zeros(0, np.uint32), np.zeros(0, np.uint8)).empty
        except hc.HcError:
            pass
        with pytest.raises(hc.HcError) as e:
            sc.fno1_from_graph(None)
        assert e.value.status == ERR_STATE
        sc.fno1_from_graph(dev)  # the host tables still serve


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def _small(sc, seed=31, V=300, n_srs=40):
    a, b = _trans.interval_edges(V, 4, seed=seed)
    tables = R.seeded_tables(seed + 1, V, n_srs)
    R.load(sc, R.graph_records(a, b, tables[0], seed + 2), V)
    return tables


def test_what_the_device_does_not_decide_and_what_is_refused():
    with hc.EdgeScorer() as sc:
        tables = R.seeded_tables(30, 300, 40)
        with pytest.raises(hc.HcError) as e:  # no graph
            sc.fno1_from_graph(tables)
        assert e.value.status == ERR_STATE
        tables = _small(sc)
        inp, text, counters = R.expected(sc, tables)
        good = sc.fno1_from_graph(tables)
        R.assert_same_run(sc, good, inp, text, counters, "small")
        for flags in (F.ADD_DUPLICATES, F.RESOLVE_ORIENTATIONS | 1 << 7):
            with pytest.raises(hc.HcError) as e:
                sc.fno1_from_graph(tables, flags=flags)
            assert e.value.status == ERR_ARG
        # new_read_count = 10^10 + 1: ids beyond the keys; hc_fno1_run on the fetched arrays answers as ever
        big = tables[:6] + (10 ** 10 + 1,)
        with pytest.raises(hc.HcError) as e:
            sc.fno1_from_graph(big)
        assert e.value.status == NOT_ON_DEVICE
        assert R.expected(sc, big)[1] == text
        # a perc of 1000 on a stored non-edge between two unvisited vertices
        free = np.flatnonzero(tables[0]["visited"] == 0)
        u, v = int(free[0]), int(free[-1])
        ne = R.seeded_nonedges(33, 50, tables[0], inp.graph_edges)
        ne[7]["v1"], ne[7]["v2"], ne[7]["perc"], ne[7]["ord"], ne[7]["pos2"], ne[7]["len2"] = u, v, 1000, ord("-"), 0, 0
        joined = {(int(x["v1"]), int(x["v2"])) for x in inp.graph_edges}
        assert (u, v) not in joined and (v, u) not in joined and not tables[0]["paired"][u] and not tables[0]["paired"][v]
        with pytest.raises(hc.HcError) as e:
            sc.fno1_from_graph(tables, ne)
        assert e.value.status == NOT_ON_DEVICE
        _, text_ne, _ = R.expected(sc, tables, ne)
        assert b"\t1000\t0\t" in text_ne
        # ... and nothing was changed: the fetches still hand out the last good call's
        sc._fno1 = good
        assert sc.fno1_text() == text and sc.fno1_edges()[1] == [len(inp.graph_edges), 0, 0, 0]


def test_zero_edges_is_an_empty_text():
    with hc.EdgeScorer() as sc:
        tables = R.seeded_tables(40, 50, 5)
        R.load(sc, np.zeros(0, host.EDGE_DTYPE), 50)
        res = sc.fno1_from_graph(tables)
        assert res.counts["n_lines"] == res.counts["n_bytes"] == res.counts["n_items"] == 0
        assert sc.fno1_text() == b"" and sc.fno1_edges()[1] == [0, 0, 0, 0] and sc.fno1_lines_device()[1] == 0


# ---- 6. determinism and scale ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes_on_a_graph_of_300000_records():
    V = 60000
    a, b = _trans.interval_edges(V, 7, seed=50)
    assert 290000 < len(a) < 360000
    tables = R.seeded_tables(51, V, 6000)
    recs = R.graph_records(a, b, tables[0], 52)
    incl = (np.random.default_rng(53).random(V) < 0.01).astype(np.uint8)
    with hc.EdgeScorer() as sc:
        R.load(sc, recs, V, incl)
        sc.graph_remove_inclusions()
        edges = F.edges_from_graph(sc.graph_fetch()["edges"])
        nonedges = R.seeded_nonedges(54, 100000, tables[0], edges)
        inp, text, counters = R.expected(sc, tables, nonedges)
        first = sc.fno1_from_graph(tables, nonedges)
        R.assert_same_run(sc, first, inp, text, counters, "3e5 records")
        lines = _lines_of(sc)[2]
        second = sc.fno1_from_graph(tables, nonedges)
        assert sc.fno1_text(piece_bytes=1 << 20) == text and _lines_of(sc)[2].tobytes() == lines.tobytes()
        assert first.counts["n_lines"] == second.counts["n_lines"] > 100000 and first.counts["n_induced"] > 0
