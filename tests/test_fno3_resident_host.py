"""hc_host_fno3_from_originals (include/hcsr.h), the host mirror of FNO=3 from the kept dict: against the restatement of the rule in
tests/_fno3_resident.py on seeded dicts (text byte for byte, counters, candidate table; some seeds with about a fifth of the pairs
ambiguous), against the reference's eight whole runs (every unambiguous pair writes the reference's line), against hc_fno3_run and the
oracle on scenarios in which every shared original of a pair agrees, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from haploconduct_amd import _native as N
from haploconduct_amd import fno as F
from haploconduct_amd import host
from haploconduct_amd import originals as OR
from tests import _fno as T
from tests import _fno3_resident as R

BIG = 10 ** 9

# seed, (n_single, n_trivial, n_paired), originals, share of moved entries, paired originals
SEEDED = [
    (11, (12, 10, 8), 60, 0.0, True),
    (12, (30, 25, 20), 200, 0.05, True),
    (13, (100, 120, 80), 700, 0.07, False),
    (14, (0, 40, 0), 90, 0.3, True),       # trivials only, single-end and paired
    (15, (25, 0, 25), 150, 0.03, True),    # no trivials
    (16, (40, 30, 0), 150, 0.0, False),    # no pairs
    (17, (60, 60, 60), 500, 0.6, True),
]


@pytest.mark.parametrize("seed,counts3,n_orig,perturb,paired_originals", SEEDED)
@pytest.mark.parametrize("flags", [0, F.NO_INCLUSIONS])
def test_mirror_equals_the_restatement(seed, counts3, n_orig, perturb, paired_originals, flags):
    off, entries, reads = R.window_scenario(seed, counts3, n_orig, perturb=perturb, paired_originals=paired_originals, share=(1, 2, 3, 5, 9))
    assert 30 <= len(reads) <= 300
    got = host.fno3_from_originals(off, entries, reads, counts3, BIG, flags=flags)
    R.same(got, R.restate(off, entries, reads, counts3, BIG, flags=flags), f"seed {seed}")
    assert got.counts["candidates"] > 20 and got.counts["n_lines"] > 5 and got.counts["n_combos"] > got.counts["candidates"]
    frac = got.counts["n_ambiguous"] / got.counts["candidates"]
    if 0 < perturb < 0.1:
        assert 0.12 <= frac <= 0.3, frac  # about a fifth (a property of the seed, fixed here so that it stays one)
    elif perturb == 0:
        assert frac == 0


def test_the_seeds_hold_every_branch_and_walk_ranks_reorder_the_pairs():
    off, entries, reads = R.window_scenario(12, (30, 25, 20), 200, perturb=0.05)
    got = host.fno3_from_originals(off, entries, reads, (30, 25, 20), BIG)
    types = {tuple(l.split(b"\t")[11:13]) for l in got.text.split(b"\n")[:-1]}
    assert types == {(b"s", b"s"), (b"p", b"s"), (b"s", b"p"), (b"p", b"p")}
    # a paired super-read with a single-end trivial behind it: the pair is SR1 although its id is the larger one
    rank = R.ranks((30, 25, 20))
    ps = [c for c in got.candidates if reads[c["a"]]["paired"] and not reads[c["b"]]["paired"] and c["a"] > c["b"]]
    assert ps and all(rank[c["a"]] < rank[c["b"]] and 30 <= c["b"] < 55 and c["a"] >= 55 for c in ps)
    # an explicit rank that is not monotone: same pairs, another SR1 for some, another order
    walk = np.random.default_rng(3).permutation(len(reads)).astype(np.uint32)
    other = host.fno3_from_originals(off, entries, reads, (30, 25, 20), BIG, walk_rank=walk)
    R.same(other, R.restate(off, entries, reads, (30, 25, 20), BIG, walk_rank=walk), "explicit walk_rank")
    pairs = lambda res: {frozenset((int(c["a"]), int(c["b"]))) for c in res.candidates}
    assert pairs(other) == pairs(got) and [tuple(c)[:2] for c in other.candidates] != [tuple(c)[:2] for c in got.candidates]
    assert all(walk[c["a"]] < walk[c["b"]] for c in other.candidates)
    keys = [(int(walk[c["a"]]), int(walk[c["b"]])) for c in other.candidates]
    assert keys == sorted(keys)


def test_golden_runs_every_unambiguous_pair_writes_the_references_line():
    cases = R.golden_cases()
    assert len(cases) == 8
    for c, off, entries, reads, counts3 in cases:
        n = len(reads)
        got = host.fno3_from_originals(off, entries, reads, counts3, c["original_readcount"], walk_rank=np.arange(n, dtype=np.uint32), flags=c["flags"])
        srs = np.zeros(n, F.FNO_READ_DTYPE)
        srs[:] = reads
        oo = np.asarray(c["orig_off"])
        orig = np.zeros(len(c["originals_in_iteration_order"]), F.FNO_ORIGINAL_DTYPE)
        for k, o in enumerate(c["originals_in_iteration_order"]):
            orig[k] = tuple(o)
        inp = F.Fno3Input(srs, *c["counts"], [orig[oo[i]:oo[i + 1]] for i in range(n)], new_read_count=c["new_read_count"],
                          original_readcount=c["original_readcount"], flags=c["flags"])
        text, cn = F.find_next_overlaps3(inp)
        assert text == c["text"].encode()
        assert got.counts["candidates"] == cn["candidates"] == len(got.candidates)
        gold, mine = R.lines_by_pair(text), R.lines_by_pair(got.text)
        pair_of = lambda cd: frozenset((int(reads[cd["a"]]["id"]), int(reads[cd["b"]]["id"])))
        listed = {pair_of(cd) for cd in got.candidates}
        assert len(listed) == len(got.candidates) and set(gold) <= listed and set(mine) <= listed
        n_amb = n_lines = 0
        for cd in got.candidates:
            if cd["flags"] & OR.CAND_AMBIGUOUS:
                n_amb += 1
                continue
            assert mine.get(pair_of(cd)) == gold.get(pair_of(cd)), (sorted(pair_of(cd)), mine.get(pair_of(cd)), gold.get(pair_of(cd)))
            assert bool(cd["flags"] & OR.CAND_LINE) == (pair_of(cd) in mine)
            n_lines += pair_of(cd) in mine
        print(f"golden run: {len(got.candidates)} pairs, {n_amb} ambiguous ({100 * n_amb / len(got.candidates):.1f} %), {n_lines} unambiguous lines")
        assert n_amb == got.counts["n_ambiguous"] and 4 * n_amb <= len(got.candidates) and n_lines >= 30


@pytest.mark.parametrize("seed,paired_originals", [(21, True), (22, False), (23, True)])
@pytest.mark.parametrize("flags", [0, F.NO_INCLUSIONS])
def test_consistent_scenarios_equal_fno3_run_and_the_oracle(seed, paired_originals, flags):
    counts3 = (25, 20, 15)
    off, entries, reads = R.window_scenario(seed, counts3, 160, paired_originals=paired_originals)
    got = host.fno3_from_originals(off, entries, reads, counts3, BIG, flags=flags)
    assert got.counts["n_ambiguous"] == 0 and got.counts["n_lines"] > 30
    inp = R.fno3_input(off, entries, reads, counts3, 160, flags=flags, seed=seed)  # (the reference sizes nodes_to_SR by it)
    runs = [F.find_next_overlaps3(inp)]
    if os.path.exists(T.ORACLE_LIB):
        runs.append(T.oracle_fno3(T.load_oracle(), inp))
    for text, cn in runs:
        assert sorted(text.split(b"\n")) == sorted(got.text.split(b"\n"))
        assert cn["candidates"] == got.counts["candidates"] and cn["n_lines"] == got.counts["n_lines"]


def test_inclusions_at_exactly_100_percent_are_dropped_by_the_flag_only():
    # read 1 lies inside read 0 (perc 100), read 2 overlaps read 0 by 99 of its 100 bases, reads 1 and 2 do not meet
    maps = [[(5, 0, 0, 50, 0, 0)], [(5, -30, 0, 50, 0, 0)], [(5, 0 - 201, 0, 50, 0, 0)]]
    off, entries = R.to_csr(maps)
    reads = R.make_reads([(300, 0, 0), (100, 0, 0), (100, 0, 0)])
    plain = host.fno3_from_originals(off, entries, reads, (3, 0, 0), BIG)
    strict = host.fno3_from_originals(off, entries, reads, (3, 0, 0), BIG, flags=F.NO_INCLUSIONS)
    R.same(plain, R.restate(off, entries, reads, (3, 0, 0), BIG))
    R.same(strict, R.restate(off, entries, reads, (3, 0, 0), BIG, flags=F.NO_INCLUSIONS))
    percs = lambda res: sorted(int(l.split(b"\t")[7]) for l in res.text.split(b"\n")[:-1])
    assert percs(plain) == [99, 100] and percs(strict) == [99] and len(plain.candidates) == 3
    assert [int(c["flags"]) & OR.CAND_LINE for c in strict.candidates].count(0) == 2


def _status(fn):
    with pytest.raises(N.HcError) as e:
        fn()
    return e.value.status


def test_refusals():
    counts3 = (12, 10, 8)
    off, entries, reads = R.window_scenario(11, counts3, 60)
    ok = host.fno3_from_originals(off, entries, reads, counts3, BIG)
    run = lambda **kw: host.fno3_from_originals(off, entries, reads, kw.pop("counts3", counts3), kw.pop("original_readcount", BIG), **kw)
    # HC_ERR_ARG: counts that do not add up, a rank that is no permutation, bits nobody defined, max_combos beyond the limit
    assert _status(lambda: run(counts3=(12, 10, 9))) == -1
    assert _status(lambda: run(counts3=(12, 10, 2 ** 64 - 22))) == -1
    dup = np.arange(30, dtype=np.uint32)
    dup[7] = 8
    assert _status(lambda: run(walk_rank=dup)) == -1
    far = np.arange(30, dtype=np.uint32)
    far[29] = 30
    assert _status(lambda: run(walk_rank=far)) == -1
    assert _status(lambda: run(flags=0x10)) == -1
    assert _status(lambda: run(max_combos=2 ** 31 - 15)) == -1
    # the other known bits are accepted and ignored, as hc_fno3_run takes them
    R.same(run(flags=F.RESOLVE_ORIENTATIONS | F.OPTIMIZE | F.ADD_DUPLICATES), ok)
    # HC_ERR_FORMAT: more distinct originals than original_readcount (nodes_to_SR.at)
    assert ok.counts["n_originals"] == 60
    R.same(run(original_readcount=60), ok)
    assert _status(lambda: run(original_readcount=59)) == -9
    with pytest.raises(R.Stop):
        R.restate(off, entries, reads, counts3, 59)
    # HC_ERR_NOT_ON_DEVICE: one combination more than allowed
    R.same(run(max_combos=ok.counts["n_combos"]), ok)
    assert _status(lambda: run(max_combos=ok.counts["n_combos"] - 1)) == -11
    # a read of length 0, ids that do not ascend inside a read
    empty = reads.copy()
    empty["len1"][3] = 0
    assert _status(lambda: host.fno3_from_originals(off, entries, empty, counts3, BIG)) == -1
    k = int(np.flatnonzero(np.diff(off.astype(np.int64)) >= 2)[0])
    swapped = entries.copy()
    swapped[[int(off[k]), int(off[k]) + 1]] = swapped[[int(off[k]) + 1, int(off[k])]]
    assert _status(lambda: host.fno3_from_originals(off, swapped, reads, counts3, BIG)) == -1


def test_count_then_fetch_and_null_arguments():
    counts3 = (12, 10, 8)
    off, entries, reads = R.window_scenario(11, counts3, 60)
    want = host.fno3_from_originals(off, entries, reads, counts3, BIG)
    inp = OR.hc_fno3_resident_input(*counts3, None, BIG, 0, 0, 0)
    cn, nb = OR.hc_fno3_resident_counts(), C.c_uint64()
    call = lambda text, cap, cands, cap_cands: N.lib.hc_host_fno3_from_originals(off.ctypes.data, entries.ctypes.data, 30, reads.ctypes.data, C.byref(inp),
                                                                                 C.byref(cn), text, cap, C.byref(nb), cands, cap_cands)
    assert call(None, 0, None, 0) == -1 and nb.value == cn.n_bytes == len(want.text) and cn.candidates == len(want.candidates)
    text, cands = np.full(nb.value + 1, 0x55, np.uint8), np.zeros(cn.candidates, OR.FNO3_CANDIDATE_DTYPE)
    assert call(text.ctypes.data, nb.value - 1, cands.ctypes.data, cands.size) == -1 and (text == 0x55).all()  # too small: nothing copied
    assert call(text.ctypes.data, nb.value, cands.ctypes.data, cands.size - 1) == -1 and (text == 0x55).all()
    assert call(text.ctypes.data, nb.value, cands.ctypes.data, cands.size) == 0
    assert text[:-1].tobytes() == want.text and text[-1] == 0x55 and cands.tobytes() == want.candidates.tobytes()
    for args in ((None, entries.ctypes.data, 30, reads.ctypes.data, C.byref(inp), C.byref(cn), None, 0, C.byref(nb), None, 0),
                 (off.ctypes.data, entries.ctypes.data, 30, None, C.byref(inp), C.byref(cn), None, 0, C.byref(nb), None, 0),
                 (off.ctypes.data, entries.ctypes.data, 30, reads.ctypes.data, None, C.byref(cn), None, 0, C.byref(nb), None, 0),
                 (off.ctypes.data, entries.ctypes.data, 30, reads.ctypes.data, C.byref(inp), None, None, 0, C.byref(nb), None, 0),
                 (off.ctypes.data, entries.ctypes.data, 30, reads.ctypes.data, C.byref(inp), C.byref(cn), None, 0, None, None, 0)):
        assert N.lib.hc_host_fno3_from_originals(*args) == -1
    # nothing shared: no combination, no candidate, an empty text, and HC_OK without any buffer
    maps = [[(r, 0, 0, 50, 0, 0)] for r in range(5)] + [[]]
    off2, entries2 = R.to_csr(maps)
    none = host.fno3_from_originals(off2, entries2, R.make_reads([(100, 0, 0)] * 6), (6, 0, 0), BIG)
    assert none.text == b"" and none.counts["n_combos"] == 0 and none.counts["candidates"] == 0 and none.counts["n_originals"] == 5
