"""Super-read consensus on the device (hc_sr_consensus, include/hcsr.h) against the reference's golden vectors and, at sizes no
golden file holds, against the host mirror: byte for byte, return values and statuses included.  More than 10^5 layouts in all."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import consensus as SR
from haploconduct_amd import host, synth
from haploconduct_amd.readstore import ReadSet
from tests import _sr

pytestmark = pytest.mark.gpu


def _both(sc, reads, layouts, members, **kw):
    dev = sc.sr_consensus(layouts, members, **kw)
    ref = host.sr_consensus(reads, layouts, members, n_threads=16, **kw)
    return dev, ref


def test_device_equals_every_golden_case():
    with hc.EdgeScorer() as sc:
        def run(reads, layouts, members, min_qual, mcs, ec, sub):
            sc.set_reads(reads)
            return sc.sr_consensus(layouts, members, min_qual, mcs, ec, sub)

        assert _sr.check_against_golden(run) >= 150


def _edges_from_candidates(cand, n_reads):
    e = np.zeros(cand.size, host.EDGE_DTYPE)
    for k in ("read1", "read2", "ori1", "ori2", "pos1"):
        e[k] = cand[k]
    e["v1"] = cand["read1"].astype(np.uint64) + np.where(cand["ori1"] != 0, 0, n_reads).astype(np.uint64)
    e["v2"] = cand["read2"].astype(np.uint64) + np.where(cand["ori2"] != 0, 0, n_reads).astype(np.uint64)
    return e


def test_edge_merges_of_single_end_reads_never_reach_the_host():
    """(a) Layouts built by the helper from a synthetic graph's edges.  Every column has one or two members, and those come from the
    host-built table: the host finishes ZERO columns by design."""
    reads, meta = synth.make_single_dataset(20000, 30000, seed=31)
    cand = synth.single_candidates(meta, min_overlap=60, n_candidates=60000, seed=32)
    edges = _edges_from_candidates(cand, reads.n_reads)
    layouts, members = host.sr_edge_layouts(edges, reads)
    assert layouts.size >= 55000 and {0, 1} <= set(np.unique(members["rev"]))
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        for ec in (False, True):
            dev, ref = _both(sc, reads, layouts, members, error_correction=ec)
            _sr.assert_same(dev, ref, f"edge merges, error_correction={ec}")
            assert dev.n_host_columns == 0
            assert (dev.status == SR.SR_OK).mean() > 0.9 and dev.n_columns > 150 * 0.9 * layouts.size * (0.3 if ec else 1)
            print(f"edge merges ec={ec}: {layouts.size} layouts, {dev.n_columns} columns, host-finished {dev.n_host_columns}")


def test_random_cliques_of_depth_3_to_64():
    """(b) equality only; the host-finished share is printed."""
    reads, _ = synth.make_paired_dataset(3000, 8000, flip_frac=0.25, seed=41)
    singles, _ = synth.make_single_dataset(3000, 8000, seed=42)
    s = [singles.seq(q) for q in range(singles.n_seq)]
    p = [(reads.seq(2 * r), reads.seq(2 * r + 1)) for r in range(reads.n_reads)]
    both = ReadSet.from_lists(s, p)
    rng = np.random.default_rng(43)
    layouts, members = _sr.random_cliques(rng, both, 20000, 3, 64)
    with hc.EdgeScorer() as sc:
        sc.set_reads(both)
        for kw in (dict(error_correction=True, min_clique_size=4), dict(error_correction=False), dict(error_correction=True, min_qual=0.9, min_clique_size=2),
                   dict(error_correction=True, subreads_needed=True, min_clique_size=7)):
            dev, ref = _both(sc, both, layouts, members, **kw)
            _sr.assert_same(dev, ref, f"cliques {kw}")
            assert dev.n_columns > 0
            print(f"cliques {kw}: {dev.n_columns} columns, host-finished {dev.n_host_columns} ({100.0 * dev.n_host_columns / dev.n_columns:.2f} %)")


def test_cliques_of_reads_that_agree_are_mostly_finished_on_the_device():
    """Cliques of reads that tile one place of a genome: most columns of depth >= 3 fall into the region the device decides by
    comparisons (Phred 93).  Equality with the mirror is the assertion; the share is printed."""
    reads, meta = synth.make_single_dataset(6000, 15000, flip_frac=0.0, n_strains=1, seed=71)
    rng = np.random.default_rng(72)
    order = np.argsort(meta["s"], kind="stable")
    n, depth = 12000, 12
    idx = order[rng.integers(0, reads.n_reads - depth, n)[:, None] + np.arange(depth)[None, :]]
    pos = meta["s"][idx] - meta["s"][idx][:, :1]
    members = np.zeros(n * depth, SR.SR_MEMBER_DTYPE)
    members["read"], members["pos"] = idx.ravel(), pos.ravel()
    layouts = np.zeros(n, SR.SR_LAYOUT_DTYPE)
    layouts["first_member"], layouts["n_members"], layouts["total_len"] = np.arange(n) * depth, depth, (pos + 150).max(axis=1)
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        for kw in (dict(error_correction=True, min_clique_size=4), dict(error_correction=False, min_qual=0.9)):
            dev, ref = _both(sc, reads, layouts, members, **kw)
            _sr.assert_same(dev, ref, f"agreeing cliques {kw}")
            assert (dev.status == SR.SR_OK).mean() > 0.5
            print(f"agreeing cliques {kw}: {dev.n_columns} columns, host-finished {dev.n_host_columns} ({100.0 * dev.n_host_columns / dev.n_columns:.2f} %)")


@pytest.mark.parametrize("K", [6, 35, 60, 70])
def test_every_store_encoding_and_both_orientations(K):
    """(c) narrow, the two wide 8-bit encodings and 16-bit symbols."""
    quals = [33 + q for q in np.linspace(2, 93, K).round().astype(int)] if K > 42 else [35 + q for q in range(K)]
    assert len(set(quals)) == K
    reads, _ = synth.make_single_dataset(4000, 6000, seed=50 + K, quals=quals, n_rate=0.01)
    rng = np.random.default_rng(K)
    layouts, members = _sr.random_cliques(rng, reads, 6000, 1, 7)
    assert {0, 1} <= set(np.unique(members["rev"]))
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        assert sc.info()["qual_alphabet"] == K
        for ec in (False, True):
            dev, ref = _both(sc, reads, layouts, members, error_correction=ec, min_clique_size=3)
            _sr.assert_same(dev, ref, f"K={K} ec={ec}")
            assert (dev.status == SR.SR_OK).any()


def test_mixed_lengths():
    """(d) lengths from 60 to 3000 bases, log-uniform."""
    reads, _ = synth.make_single_dataset(3000, 20000, len_lo=60, len_hi=3000, log_uniform=True, seed=61)
    rng = np.random.default_rng(62)
    layouts, members = _sr.random_cliques(rng, reads, 8000, 2, 12)
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        for ec in (False, True):
            dev, ref = _both(sc, reads, layouts, members, error_correction=ec, min_clique_size=2)
            _sr.assert_same(dev, ref, f"mixed lengths ec={ec}")
            assert (dev.status == SR.SR_OK).any()


def test_malformed_layouts_and_invalid_symbols_on_the_device():
    reads = ReadSet.from_lists([("ACGTACGTAC", "IIIIIIIIII"), ("ACGTXCGTAC", "IIIIIIIIII"), ("ACGTACGTAC", "IIII\x1fIIIII")],
                               [(("ACGTACGT", "IIIIIIII"), ("TTTTCCCC", "55555555"))])
    rows = [[(0, 0, 0, 0)], [(9, 0, 0, 0)], [(0, 0, 0, 1)], [(0, 0, 0, 0), (0, 0, 0, 5), (0, 0, 0, 3)], [(0, 1, 0, 0)], [(3, 0, 0, 0)], [(0, 0, 2, 0)],
            [(1, 0, 0, 0)], [(2, 0, 1, 0)], [(3, 1, 0, 0), (3, 2, 1, 0)], [(0, 0, 0, 0), (0, 0, 0, 0)]]
    total = [10, 10, 11, 15, 10, 10, 10, 10, 10, 8, 9]
    members = np.array([(r, p, s, v, (0, 0)) for row in rows for r, s, v, p in row], SR.SR_MEMBER_DTYPE)
    layouts = np.zeros(len(rows) + 2, SR.SR_LAYOUT_DTYPE)
    k = 0
    for i, row in enumerate(rows):
        layouts[i] = (k, len(row), total[i])
        k += len(row)
    layouts[-2] = (k, 1, 10)        # first_member past the end
    layouts[-1] = (0, 2**32 - 1, 10)  # more members than there are
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        dev, ref = _both(sc, reads, layouts, members, min_qual=0.5)
    _sr.assert_same(dev, ref, "malformed")
    B, S = SR.SR_BAD_LAYOUT, SR.SR_BAD_SYMBOL
    assert list(dev.status) == [0, B, B, B, B, B, B, S, S, 0, B, B, B]


def test_count_then_fetch():
    import ctypes as C

    from haploconduct_amd import _native as N

    reads, _ = synth.make_single_dataset(50, 2000, seed=7)
    layouts, members = _sr.random_cliques(np.random.default_rng(8), reads, 20, 2, 5)
    with hc.EdgeScorer() as sc:
        sc.set_reads(reads)
        full = sc.sr_consensus(layouts, members)
        st = SR.make_settings()
        ret, status, off, nb = np.zeros(20, np.int32), np.zeros(20, np.uint32), np.zeros(21, np.uint64), C.c_uint64()
        rc = N.lib.hc_sr_consensus(sc._ctx, layouts.ctypes.data, 20, members.ctypes.data, members.size, C.byref(st), ret.ctypes.data,
                                   status.ctypes.data, off.ctypes.data, None, None, 0, C.byref(nb), None)
        assert rc != 0 and nb.value == full.cons_seq.size and np.array_equal(off, full.out_off) and np.array_equal(ret, full.ret)
