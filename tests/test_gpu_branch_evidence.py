"""hc_br_evidence on the device against its host mirror (hc_host_br_evidence), table by table and status by status, for equality.  Graphs come
through hc_graph_load, the dict through hc_sr_originals_load, the reads through set_reads with keeping on.  The shapes are the smallest at
which each kernel can go wrong: branch counts around a wave, neighbour counts up to a list of 70, overlaps around the 64-position step of the
pair wave, the 100-position cap, dict sizes around a wave, item totals around a block, diff lists of 1 and of more than 64 positions."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import branch_evidence as BR
from tests import _branch_evidence as T

pytestmark = pytest.mark.gpu

GOLDEN, _ = T.golden_cases()
STATUS = T.status_cases()


@pytest.fixture(scope="module")
def scorer():
    with hc.EdgeScorer(hc.Settings(edge_threshold=0.97, min_overlap_len=10)) as sc:
        sc.sr_keep_device(True)
        yield sc


def load(sc, case):
    g = case.graph()
    sc.set_reads(case.reads())
    sc.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
    sc.sr_originals_load(*case.dict_arrays())
    sc.br_set_original_reads(*case.original_arrays())
    return g


def device_run(sc, case):
    load(sc, case)
    counts = sc.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    res = sc.br_evidence_fetch()
    res.counts = counts
    return res


def check(sc, case):
    dev, mirror = device_run(sc, case), T.host_run(case)
    assert dev.counts.pop("ms_device") >= 0 and mirror.counts.pop("ms_device") == 0
    T.assert_same_tables(dev, mirror)
    return dev


@pytest.mark.parametrize("k", range(len(GOLDEN)), ids=[c.name for c, _ in GOLDEN])
def test_device_equals_the_mirror_and_the_reference_on_every_golden_case(scorer, k):
    case, want = GOLDEN[k]
    dev = check(scorer, case)
    assert T.as_expected(dev) == want


@pytest.mark.parametrize("name", sorted(STATUS))
def test_statuses(scorer, name):
    case, statuses = STATUS[name]
    dev = check(scorer, case)
    assert {(int(b["node"]), int(b["side"])): int(b["status"]) for b in dev.branches if b["status"] != BR.BR_OK} == statuses
    assert dev.counts["some_failed"]


@pytest.mark.parametrize("n_branches", [1, 63, 64, 65])
def test_branch_counts_around_a_wave(scorer, n_branches):
    fans = [dict(k=2, L=20 + b % 5, diffs=[[], [b % 7, 9]], dict_sizes=[1, b % 3], side="in" if b % 4 == 1 else "out", fwd=b % 3 != 0) for b in range(n_branches)]
    dev = check(scorer, T.fan_case(40 + n_branches, fans))
    assert dev.counts["n_branches"] == n_branches


def test_neighbour_counts_2_3_12_and_70(scorer):
    def diffs(k, L):
        return [[]] + [[(7 * j) % L, (11 * j + 3) % L] for j in range(1, k)]

    fans = [dict(k=2, L=40, diffs=diffs(2, 40), dict_sizes=[2, 2]), dict(k=3, L=40, diffs=diffs(3, 40), dict_sizes=[1, 2, 3], side="in"),
            dict(k=12, L=50, diffs=diffs(12, 50), dict_sizes=[2] * 12, shift=1), dict(k=70, L=80, diffs=diffs(70, 80), dict_sizes=[1] * 70),
            dict(k=70, L=80, diffs=diffs(70, 80), dict_sizes=[0] * 70, side="in", fwd=0)]
    dev = check(scorer, T.fan_case(51, fans))
    assert sorted(int(b["n_neighbours"]) for b in dev.branches) == [2, 3, 12, 70, 70]


@pytest.mark.parametrize("L", [1, 63, 64, 65, 129, 1000])
def test_overlap_lengths_with_the_first_difference_at_the_front_at_the_back_and_none(scorer, L):
    fans = []
    for side in ("out", "in"):
        for fwd in (1, 0):
            fans += [dict(k=2, L=L, diffs=[[], [0]], dict_sizes=[3, 3], side=side, fwd=fwd), dict(k=2, L=L, diffs=[[], [L - 1]], dict_sizes=[3, 3], side=side, fwd=fwd),
                     dict(k=2, L=L, diffs=[[], []], dict_sizes=[2, 2], side=side, fwd=fwd)]
    dev = check(scorer, T.fan_case(60 + L, fans, min_overlap_len=0))  # (an overlap of 1 is below any other min_overlap_len)
    assert dev.counts["n_missing"] == 4 and int(dev.branches["is_false"].sum()) == 4


@pytest.mark.parametrize("n_diff", [99, 100, 101])
def test_the_100_position_cap(scorer, n_diff):
    pos = [3 * i + 1 for i in range(n_diff)]
    fans = [dict(k=2, L=400, diffs=[[], pos], dict_sizes=[4, 4], side=side) for side in ("out", "in")]
    dev = check(scorer, T.fan_case(70 + n_diff, fans))
    assert dev.branches["diff_count"].tolist() == [min(n_diff, 100)] * 2


def test_relative_pos_at_the_inclusion_threshold_and_one_beyond(scorer):
    rng = np.random.default_rng(81)
    a, b, c = T.random_seq(rng, 80), T.random_seq(rng, 30), T.random_seq(rng, 60)
    # neighbour 1 (30 bases, min_overlap_len 10) at pos 5; neighbour 2 at 5 + 20 (the threshold) and at 5 + 21 (a missing inclusion pair)
    for shift, cleared in ((20, False), (21, True)):
        case = T.Case(f"threshold{shift}", [a, b, c], [0, 1, 2], [1, 1, 1], [(0, 1, 5), (0, 2, 5 + shift)], [[], [], []], ["ACGT"], 1, 0, 1)
        dev = check(scorer, case)
        assert (int(dev.branches[0]["nb_count"]) == 0) == cleared
    # with a third neighbour the branch stays and only the included neighbour leaves
    case = T.Case("threshold_three", [a, b, c, a[7:] + c[:9]], [0, 1, 2, 3], [1] * 4, [(0, 1, 5), (0, 2, 26), (0, 3, 7)], [[]] * 4, ["ACGT"], 1, 0, 1)
    dev = check(scorer, case)
    assert dev.neighbours(0).tolist() == [2, 3]


@pytest.mark.parametrize("sizes", [(0, 1), (63, 64), (65, 300)])
def test_dict_sizes_around_a_wave(scorer, sizes):
    dev = check(scorer, T.fan_case(90 + sizes[0], [dict(k=2, L=120, diffs=[[], [5, 60, 119]], dict_sizes=list(sizes)),
                                                   dict(k=2, L=120, diffs=[[], [0, 64]], dict_sizes=list(sizes), side="in", fwd=0)]))
    assert dev.counts["n_items"] == 2 * sum(sizes)


@pytest.mark.parametrize("total", [255, 256, 257])
def test_item_totals_around_a_block(scorer, total):
    dev = check(scorer, T.fan_case(100 + total, [dict(k=3, L=90, diffs=[[], [4], [50]], dict_sizes=[100, 100, total - 200])]))
    assert dev.counts["n_items"] == total


def test_diff_lists_of_one_and_of_more_than_64_with_reads_that_cover_none_one_and_all(scorer):
    rng = np.random.default_rng(111)
    cases = []
    for n_pos in (1, 70):
        L = 300
        pos = [40 + 3 * i for i in range(n_pos)]
        common = T.random_seq(rng, L)
        n1, n2 = common, T.mutate(common, pos)
        seqs = [T.random_seq(rng, 30) + common[:10], n1, n2]
        originals, d1, d2 = [], [], []

        def add(seq, at, flip=None):
            o = seq[at[0]:at[1]]
            if flip is not None:
                o = T.mutate(o, [flip - at[0]])
            originals.append(o)
            return (len(originals) - 1, at[0], 1)

        for seq, d in ((n1, d1), (n2, d2)):
            d.append(add(seq, (0, 30)))                          # covers none
            d.append(add(seq, (pos[0] - 5, pos[0] + 1)))         # covers the first alone
            d.append(add(seq, (0, L)))                           # covers all
            d.append(add(seq, (0, L), flip=pos[0]))              # disagrees at the first covered position
            d.append(add(seq, (0, L), flip=pos[-1]))             # disagrees at the last covered position
            d.append(add(seq, (pos[-1], pos[-1] + 20)))          # covers the last alone
        cases.append(T.Case(f"cover{n_pos}", seqs, [0, 1, 2], [1, 1, 1], [(0, 1, 30), (0, 2, 30)], [sorted(d1 + d2), d1, d2], originals, len(originals), 0,
                            len(originals)))
    for case in cases:
        dev = check(scorer, case)
        ev = dev.evidence()
        assert ev[(0, 1)] == [1, 2, 5] and ev[(0, 2)] == [7, 8, 11], ev


def test_an_edge_on_both_sides_with_an_empty_intersection(scorer):
    case = T.make_case(5, n_contigs=0, n_orig_se=2, n_orig_pe=1, bubbles=1)
    # without the third original the out-branch holds the first alone and the in-branch the second alone
    third = case.se_count - 1
    case.dicts = [[x for x in d if x[0] != third] for d in case.dicts]
    dev = check(scorer, case)
    assert dev.evidence()[(0, 2)] == [] and dev.counts["n_ev_edges"] == 3


def test_graph_is_left_in_target_order_and_otherwise_unchanged(scorer):
    case = T.make_case(121, max_out=5, bubbles=1)
    before = load(scorer, case)
    assert any(np.any(np.diff(before["edges"]["v2"][int(a):int(b)].astype(np.int64)) < 0) for a, b in zip(before["out_off"][:-1], before["out_off"][1:]))
    scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    after = scorer.graph_fetch()
    for k in ("out_off", "in_nodes", "in_off"):
        assert np.array_equal(before[k], after[k]), k
    for a, b in zip(before["out_off"][:-1], before["out_off"][1:]):
        want = before["edges"][int(a):int(b)]
        want = want[np.argsort(want["v2"], kind="stable")]
        assert want.tobytes() == after["edges"][int(a):int(b)].tobytes()
    assert scorer.graph_branching_edges().size == 0


def test_second_call_after_originals_next_replaced_the_dict_and_fetch_after_graph_load(scorer):
    from haploconduct_amd import merge_next as MN
    from haploconduct_amd import originals as OR
    from haploconduct_amd.consensus import SR_LAYOUT_DTYPE
    from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE

    case = T.make_case(131, bubbles=2)
    first = check(scorer, case)
    # every vertex becomes a trivial super-read of a new store with as many reads: read r's dict moves to new read perm[r]
    V = case.n_vertices
    rng = np.random.default_rng(5)
    new_id = rng.permutation(V)
    nodes = np.zeros(V, FNO_READ_DTYPE)
    for v in range(V):
        nodes[v]["id"], nodes[v]["len1"] = new_id[v], len(case.seqs[case.vertex_read[v]])
    t = OR.Tables(np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, SR_LAYOUT_DTYPE),
                  np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, FNO_SUBREAD_DTYPE), np.full(V, MN.MN_V_TRIVIAL, np.uint32), nodes,
                  np.array(case.vertex_read, np.uint32), np.ones(V, np.uint8), V, False)
    nxt = scorer.sr_originals_next(t, None, None, None)
    assert nxt.n_failed == sum(1 for d in case.dicts if not d)  # (a trivial whose read has no original: HC_SR_ORIG_EMPTY_SOURCE, and no entries)
    off, entries = scorer.sr_originals_fetch()
    moved = T.Case("moved", case.seqs, case.vertex_read, case.vertex_fwd, case.edges,
                   [[(int(e["id"]), int(e["index1"]), int(e["forward"])) for e in entries[int(off[r]):int(off[r + 1])]] for r in range(V)], case.originals,
                   case.se_count, case.pe_count, case.original_readcount)
    counts = scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())  # the same context, the replaced dict
    second = scorer.br_evidence_fetch()
    second.counts = counts
    mirror = T.host_run(moved)
    second.counts.pop("ms_device"), mirror.counts.pop("ms_device")
    T.assert_same_tables(second, mirror)
    assert second.ev_ids.tobytes() != first.ev_ids.tobytes() or second.ev_off.tobytes() != first.ev_off.tobytes()
    # the tables go with the graph
    g = case.graph()
    scorer.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
    with pytest.raises(N.HcError) as e:
        scorer.br_evidence_fetch()
    assert e.value.status == -5  # HC_ERR_STATE


def test_refusals(scorer):
    case = T.make_case(141, n_contigs=12)
    load(scorer, case)
    st = case.settings()
    st.se_count += 1
    with pytest.raises(N.HcError) as e:
        scorer.br_evidence(case.vertex_read, case.vertex_fwd, st)
    assert e.value.status == -1
    with pytest.raises(N.HcError) as e:
        scorer.br_evidence(case.vertex_read[:-1], case.vertex_fwd[:-1], case.settings())
    assert e.value.status == -1
    with hc.EdgeScorer(hc.Settings(edge_threshold=0.97, min_overlap_len=10)) as other:  # keeping is off: no kept store
        g = case.graph()
        other.set_reads(case.reads())
        other.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
        with pytest.raises(N.HcError) as e:
            other.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
        assert e.value.status == -5
    # a record that names a read outside the store, behind a paired neighbour: refused like the mirror refuses it, not a status
    case, g = T.paired_then_bad_read()
    load(scorer, case)
    scorer.graph_load(g["edges"], g["out_off"], g["in_nodes"], g["in_off"])
    with pytest.raises(N.HcError) as e:
        scorer.br_evidence(case.vertex_read, case.vertex_fwd, case.settings())
    assert e.value.status == -1

