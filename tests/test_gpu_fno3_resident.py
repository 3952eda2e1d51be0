"""hc_fno3_from_originals on the device (include/hcsr.h) against its host mirror — the text byte for byte, the counters and the candidate
table — at the shapes where a kernel's last workgroup, a bisection step, a run boundary or the packed key's shift changes: originals shared
by 1, 2, 63, 64, 65 and 300 reads, pairs sharing 1, 2, 63, 64 and 65 originals with the one disagreeing original first, last or in the
middle, stores of 1, 2, 255, 256 and 257 reads, the derived and an explicit walk rank, the inclusion filter at exactly 100 %, one of the
reference's golden runs, the refusals and what they leave in place, and one real clique iteration on one context."""
import functools

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import consensus as SR
from haploconduct_amd import fno as F
from haploconduct_amd import host
from haploconduct_amd import originals as OR
from tests import _clique_merge as CM
from tests import _edge_merge as EM
from tests import _fno3_resident as R
from tests import _originals as O

pytestmark = pytest.mark.gpu
BIG = 10 ** 9


def _device(off, entries, reads, counts3, orc=BIG, **kw):
    with hc.EdgeScorer() as sc:
        sc.set_reads(R.read_set(reads))
        sc.sr_originals_load(off, entries)
        return sc.fno3_from_originals(counts3, orc, **kw)


def _both(off, entries, reads, counts3, orc=BIG, what="", **kw):
    assert (reads["id"] == np.arange(len(reads))).all()
    ref = host.fno3_from_originals(off, entries, reads, counts3, orc, **kw)
    dev = _device(off, entries, reads, counts3, orc, **kw)
    R.same(dev, ref, what)
    return dev


def _plain_reads(n, length=400):
    return R.make_reads([(length, 0, 0)] * n)


def _groups(sizes, n_empty=0, seed=0):
    """original g is shared by sizes[g] reads of its own, each a window on one axis (no pair is ambiguous); n_empty reads have no entry"""
    rng = np.random.default_rng(seed)
    maps = []
    for g, k in enumerate(sizes):
        maps += [[(1000 + 7 * g, int(rng.integers(-150, 150)), 0, 60, 0, 0)] for _ in range(k)]
    for _ in range(n_empty):
        maps.insert(int(rng.integers(0, len(maps) + 1)), [])
    return R.to_csr(maps) + (_plain_reads(len(maps)),)


def test_originals_shared_by_1_2_63_64_65_reads_and_reads_without_an_entry():
    off, entries, reads = _groups([1, 2, 63, 64, 65, 1, 2], n_empty=9)
    dev = _both(off, entries, reads, (len(reads), 0, 0))
    c = dev.counts
    want = 1 + 63 * 62 // 2 + 64 * 63 // 2 + 65 * 64 // 2 + 1
    assert (c["n_originals"], c["n_combos"], c["candidates"], c["n_ambiguous"]) == (7, want, want, 0) and c["n_lines"] > 1000 and c["ms_device"] > 0


def test_one_hub_original_shared_by_300_reads():
    off, entries, reads = _groups([300, 3])
    dev = _both(off, entries, reads, (100, 150, 53))
    assert dev.counts["n_combos"] == dev.counts["candidates"] == 44850 + 3 and dev.counts["n_originals"] == 2


def test_no_shared_original_at_all():
    off, entries, reads = _groups([1] * 70, n_empty=5)
    dev = _both(off, entries, reads, (75, 0, 0))
    assert dev.text == b"" and dev.counts["n_combos"] == 0 and dev.counts["candidates"] == 0 and dev.counts["n_originals"] == 70
    # ... and a dict without any entry
    off, entries = R.to_csr([[] for _ in range(4)])
    dev = _both(off, entries, _plain_reads(4), (4, 0, 0))
    assert dev.text == b"" and dev.counts["n_originals"] == 0


def _runs(lengths, odd_at):
    """pair k = reads (2 k, 2 k + 1) shares lengths[k] originals that agree, except the one at place odd_at[k] of the run (None: none)"""
    maps, oid = [], 0
    for k, (n, odd) in enumerate(zip(lengths, odd_at)):
        a, b = [], []
        for j in range(n):
            a.append((oid, 40 + j, 0, 50, 0, 0))
            b.append((oid, j + (5 if odd is not None and j == odd % n else 0), 0, 50, 0, 0))
            oid += 1
        maps += [a, b]
    return R.to_csr(maps) + (_plain_reads(len(maps)),)


def test_pairs_sharing_1_2_63_64_65_originals_and_where_the_disagreeing_one_sits():
    lengths = [1, 2, 63, 64, 65, 2, 65, 65, 65, 65, 64, 130]
    odd_at = [None, None, None, None, None, 1, 0, 64, 63, 32, 63, 129]
    off, entries, reads = _runs(lengths, odd_at)
    dev = _both(off, entries, reads, (len(reads), 0, 0))
    assert dev.counts["candidates"] == len(lengths) and dev.counts["n_combos"] == sum(lengths)
    assert [int(c["flags"]) & OR.CAND_AMBIGUOUS for c in dev.candidates] == [int(o is not None) for o in odd_at]
    assert dev.counts["n_ambiguous"] == 7
    # the line is the smallest shared original's: pos1 is 40, or 35 where that one is the odd one
    assert [int(l.split(b"\t")[2]) for l in dev.text.split(b"\n")[:-1]] == [35 if o == 0 else 40 for o in odd_at]
    firsts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    assert [int(c["original_id"]) for c in dev.candidates] == firsts.tolist()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_stores_around_a_power_of_two_of_reads(n):
    counts3 = (n // 3, n // 3, n - 2 * (n // 3)) if n > 2 else (1, 0, n - 1)
    off, entries, reads = R.window_scenario(40 + n, counts3, max(2, 2 * n), perturb=0.05, share=(1, 2, 3, 5, 9), paired_trivials=0.5 if n > 2 else 0)
    dev = _both(off, entries, reads, counts3, what=f"{n} reads")
    if n > 2:
        assert dev.counts["candidates"] > n and dev.counts["n_ambiguous"] > 0
        hi = [c for c in dev.candidates if max(int(c["a"]), int(c["b"])) == n - 1]
        assert hi, "the last read takes part"
    elif n == 2:  # one single-end read and one pair that share an original or more
        assert dev.counts["candidates"] == 1


def test_derived_walk_rank_puts_a_pair_in_front_of_a_single_end_trivial_and_an_explicit_one_reorders():
    counts3 = (30, 25, 20)
    off, entries, reads = R.window_scenario(12, counts3, 200, perturb=0.05)
    dev = _both(off, entries, reads, counts3, what="derived rank")
    R.same(dev, R.restate(off, entries, reads, counts3, BIG), "derived rank, restated")
    ps = [c for c in dev.candidates if reads[c["a"]]["paired"] and not reads[c["b"]]["paired"] and c["a"] >= 55 and 30 <= c["b"] < 55]
    assert ps and any(int(c["flags"]) & OR.CAND_LINE for c in ps), "no P-S pair with a trivial behind a paired super-read"
    walk = np.random.default_rng(3).permutation(75).astype(np.uint32)
    other = _both(off, entries, reads, counts3, what="explicit rank", walk_rank=walk)
    R.same(other, R.restate(off, entries, reads, counts3, BIG, walk_rank=walk), "explicit rank, restated")
    assert other.text != dev.text and other.counts["candidates"] == dev.counts["candidates"]


def test_no_inclusions_drops_pairs_at_exactly_100_percent():
    maps = [[(5, 0, 0, 50, 0, 0)], [(5, -30, 0, 50, 0, 0)], [(5, -201, 0, 50, 0, 0)]]
    off, entries = R.to_csr(maps)
    reads = R.make_reads([(300, 0, 0), (100, 0, 0), (100, 0, 0)])
    plain = _both(off, entries, reads, (3, 0, 0))
    strict = _both(off, entries, reads, (3, 0, 0), flags=F.NO_INCLUSIONS)
    percs = lambda res: sorted(int(l.split(b"\t")[7]) for l in res.text.split(b"\n")[:-1])
    assert percs(plain) == [99, 100] and percs(strict) == [99]
    # a seeded dict with both flag values, the ignored bits set too
    counts3 = (20, 15, 12)
    off, entries, reads = R.window_scenario(5, counts3, 120, paired_originals=False)
    a = _both(off, entries, reads, counts3, flags=F.NO_INCLUSIONS | F.OPTIMIZE | F.ADD_DUPLICATES)
    b = _both(off, entries, reads, counts3)
    assert 0 < a.counts["n_lines"] < b.counts["n_lines"]


def test_a_golden_run_of_the_reference_in_a_store():
    c, off_g, entries_g, reads_g, _ = R.golden_cases()[5]  # 158 pairs, the most of the eight
    n = len(reads_g)
    ids = reads_g["id"].astype(np.int64)
    assert sorted(ids.tolist()) == list(range(n))
    at = np.argsort(ids)  # read id sits at index id
    maps = [[tuple(int(x) for x in (e["id"], e["index1"], e["index2"], 1, 1, 1)) for e in entries_g[int(off_g[i]):int(off_g[i + 1])]] for i in at]
    off, entries = R.to_csr(maps)
    reads = reads_g[at].copy()
    walk = np.zeros(n, np.uint32)
    walk[ids] = np.arange(n)
    dev = _both(off, entries, reads, (n, 0, 0), c["original_readcount"], what="golden", walk_rank=walk, flags=c["flags"])
    gold, mine = R.lines_by_pair(c["text"].encode()), R.lines_by_pair(dev.text)
    n_lines = 0
    for cd in dev.candidates:
        key = frozenset((int(cd["a"]), int(cd["b"])))
        if not cd["flags"] & OR.CAND_AMBIGUOUS:
            assert mine.get(key) == gold.get(key), sorted(key)
            n_lines += key in mine
    assert n_lines >= 30 and set(gold) <= {frozenset((int(cd["a"]), int(cd["b"]))) for cd in dev.candidates}


def _status(fn):
    with pytest.raises(hc.HcError) as e:
        fn()
    return e.value.status


def test_refusals_and_what_they_leave_in_place():
    maps, t = O.make_case(2, 40, [2, 3, 5, 8])
    off, entries = O.to_csr(maps)
    reads = _plain_reads(40)
    counts3 = (15, 15, 10)
    with hc.EdgeScorer() as sc:
        ctx = sc._ctx
        assert _status(lambda: sc.fno3_from_originals(counts3, BIG)) == -5      # no store
        sc.set_reads(R.read_set(reads))
        assert _status(lambda: OR.fno3_text(ctx, 0, 0)) == -5                   # nothing kept yet
        assert _status(lambda: sc.fno3_from_originals(counts3, BIG)) == -5      # no dict
        sc.sr_originals_load(off, entries)
        ref = host.fno3_from_originals(off, entries, reads, counts3, BIG)
        first = sc.fno3_from_originals(counts3, BIG)
        R.same(first, ref)
        assert ref.counts["n_combos"] > 3 and ref.counts["n_bytes"] > 50
        kept = lambda: R.same(OR.Fno3Resident(OR.fno3_text(ctx, 0, ref.counts["n_bytes"]), first.counts, OR.fno3_candidates(ctx, 0, ref.counts["candidates"])), ref)
        # HC_ERR_ARG: counts, rank, flags, ranges; every one leaves the text and the table of the call before
        dup = np.arange(40, dtype=np.uint32)
        dup[3] = 4
        for bad in (lambda: sc.fno3_from_originals((15, 15, 11), BIG), lambda: sc.fno3_from_originals(counts3, BIG, walk_rank=dup),
                    lambda: sc.fno3_from_originals(counts3, BIG, flags=0x10), lambda: sc.fno3_from_originals(counts3, BIG, max_combos=2 ** 31 - 15),
                    lambda: OR.fno3_text(ctx, ref.counts["n_bytes"], 1), lambda: OR.fno3_text(ctx, 1, ref.counts["n_bytes"]),
                    lambda: OR.fno3_candidates(ctx, ref.counts["candidates"], 1), lambda: OR.fno3_candidates(ctx, 2, ref.counts["candidates"] - 1)):
            assert _status(bad) == -1
            kept()
        assert OR.fno3_text(ctx, 3, 11) == ref.text[3:14] and OR.fno3_candidates(ctx, 1, 2).tobytes() == ref.candidates[1:3].tobytes()
        # HC_ERR_NOT_ON_DEVICE: one combination more than allowed; the text before is still there
        assert _status(lambda: sc.fno3_from_originals(counts3, BIG, max_combos=ref.counts["n_combos"] - 1)) == -11
        kept()
        R.same(sc.fno3_from_originals(counts3, BIG, max_combos=ref.counts["n_combos"]), ref)
        # subreads.txt's text is another text: writing it drops nothing here
        sc.sr_originals_text()
        kept()
        # HC_ERR_FORMAT: more originals than original_readcount; nothing is kept after it
        assert _status(lambda: sc.fno3_from_originals(counts3, ref.counts["n_originals"] - 1)) == -9
        assert _status(lambda: OR.fno3_text(ctx, 0, 0)) == -5
        R.same(sc.fno3_from_originals(counts3, ref.counts["n_originals"]), ref)
        # the dict is replaced: the text describes another one
        sc.sr_originals_next(t, None, None, None)
        assert _status(lambda: OR.fno3_text(ctx, 0, 0)) == -5 and _status(lambda: OR.fno3_candidates(ctx, 0, 0)) == -5
        # the new dict is over another number of reads than the store's
        n_new = len(sc.sr_originals_fetch()[0]) - 1
        assert n_new != 40 and _status(lambda: sc.fno3_from_originals((n_new, 0, 0), BIG)) == -5
        # the store is replaced: nothing is kept either
        sc.sr_originals_load(off, entries)
        sc.fno3_from_originals(counts3, BIG)
        sc.set_reads(R.read_set(reads, seed=1))
        assert _status(lambda: OR.fno3_text(ctx, 0, 0)) == -5


@functools.lru_cache(maxsize=None)
def _clique_chain():
    g = CM.seeded_cliques()
    g["csr"] = EM.csr(g["V"], g["rows"])
    g["off"], g["nodes"] = SR.clique_csr(g["cliques"])
    return g


def test_a_clique_iteration_on_one_context():
    g = _clique_chain()
    with hc.EdgeScorer() as sc:
        sc.sr_keep_device(True)
        sc.set_reads(g["reads"])
        sc.sr_originals_init()
        sc.graph_load(*g["csr"])
        merged = sc.sr_clique_merge(g["off"], g["nodes"], g["vertex_read"], g["vertex_fwd"], min_clique_size=g["m"])
        nxt = sc.sr_clique_next(g["off"], g["nodes"], merged, g["vertex_read"], g["vertex_fwd"], keep_singletons=50)
        assert not nxt.empty
        sc.sr_originals_next(nxt, merged, g["vertex_read"], g["vertex_fwd"], first_it=True)
        counts3 = (nxt.n_singles, nxt.n_trivials, nxt.n_paired)
        assert sum(counts3) == nxt.new_read_count
        dev = sc.fno3_from_originals(counts3, g["reads"].n_reads)
        off, entries = sc.sr_originals_fetch()
        reads = R.reads_of(sc.sr_next_reads_fetch())
        assert len(reads) == nxt.new_read_count and int(reads["paired"].sum()) >= nxt.n_paired
        R.same(dev, host.fno3_from_originals(off, entries, reads, counts3, g["reads"].n_reads), "clique chain")
        # the seeded cliques are disjoint, so no two new reads share an original of the first iteration: every original once, no pair
        assert dev.counts["n_originals"] == len(entries) > nxt.new_read_count and dev.counts["n_combos"] == 0 and dev.text == b""
        # the same store, its real descriptors (super-reads, trivials and pairs of the chain), under a dict whose reads do share originals
        rng = np.random.default_rng(8)
        n = nxt.new_read_count
        maps = [[] for _ in range(n)]
        for oid in range(3 * n):
            p = int(rng.random() < 0.5)
            for r in rng.choice(n, size=int(rng.integers(1, 6)), replace=False):
                maps[int(r)].append((oid, int(rng.integers(-60, 120)), int(rng.integers(-60, 120)), 80, 80, p))
        off2, entries2 = R.to_csr(maps)
        sc.sr_originals_load(off2, entries2)
        dev2 = sc.fno3_from_originals(counts3, 3 * n)
    R.same(dev2, host.fno3_from_originals(off2, entries2, reads, counts3, 3 * n), "the chain's store under a shared dict")
    assert dev2.counts["candidates"] > n and dev2.counts["n_ambiguous"] > 0 and dev2.counts["n_lines"] > n // 4
