"""Find-next-overlaps at the numeric edges of the device's sort keys: every digit count and the sign of every
column, values whose keys differ only on one side of a split between two key words, ids that are sparse and ten digits long, the
widths of the pair sort and of the nodes_to_SR sort at and past a pass boundary, and the thresholds at which a call leaves the
device.  The references are plain and know nothing of the code under test:

  R1  a scenario in which every edge is copied: the lines with Python's str(), b"".join(sorted(set(lines)))  (tests/_fno.py: copied_text)
  R2  ids are labels: the oracle on dense ids, columns 1 and 2 sent through an injective map, re-sorted as bytes for FNO=1

This file runs the scenarios through the host form (HC_FNO=host), the form every refusal of the device lands on;
tests/test_gpu_fno_numeric_edges.py runs the same cases (the case_* functions below) through both device routes.  Every comparison
is of bytes and counters, exact."""
import contextlib
import os

import pytest

from haploconduct_amd import fno as F
from tests import _fno as T

FLAG_SETS = [F.RESOLVE_ORIENTATIONS, F.RESOLVE_ORIENTATIONS | F.NO_INCLUSIONS, 0]
PAIRS = {"low ids": T.LOW_PAIR, "ten-digit ids": T.HIGH_PAIR}
NODE_COUNTS = [255, 256, 257, 65535, 65536, 65537]
PASS_BOUNDARIES = [2 ** 8, 2 ** 8 + 1, 2 ** 12, 2 ** 12 + 1, 2 ** 16, 2 ** 16 + 1]


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


@contextlib.contextmanager
def _host_form():
    saved = os.environ.get("HC_FNO")
    os.environ["HC_FNO"] = "host"
    try:
        yield
    finally:
        os.environ.pop("HC_FNO", None)
        if saved is not None:
            os.environ["HC_FNO"] = saved


def _difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"{len(g) - 1} lines for {len(w) - 1}; line {i}: {a!r} for {b!r}"
    return f"{len(g) - 1} lines for {len(w) - 1}"


def walk_level(route, new_read_count):
    """The level a call reports (fno.last_device_level) by the code's own conditions.  route: None = the host form, else what the
    on_device fixture of the GPU tests yields (2: everything on the device, 1: HC_FNO_WALK=host).  A pair of ids is sorted as
    lo << id_bits | hi, which has to fit 62 bits: past new_read_count = 2^31 the walk is the host threads'."""
    if route is None:
        return 0
    return route if new_read_count <= 2 ** 31 else 1


def check(inp, want, counters, route, level, run=F.find_next_overlaps):
    """The host form against the reference; with a route, the device against the reference, the host form's counters and the level
    the route must report, so that no silent fall-back passes."""
    with _host_form():
        h_text, h_cnt = run(inp)
        assert not F.last_on_device
    assert h_cnt == counters, (h_cnt, counters)
    assert h_text == want, "host form: " + _difference(h_text, want)
    if route is None:
        return
    got, cnt = run(inp)
    assert F.last_device_level == level, f"level {F.last_device_level} for {level}"
    assert cnt == h_cnt, (cnt, h_cnt)
    assert got == want, "device: " + _difference(got, want)


def check_copied(rows, route, level=None, new_read_count=None, flags=F.RESOLVE_ORIENTATIONS):
    inp = T.copied_scenario(rows, flags=flags, new_read_count=new_read_count)
    lines = T.copied_lines(inp)
    assert lines != sorted(lines), "the input lies in the order of the output: a stable sort that ignores a key would pass"
    want, counters = T.copied_text(inp)
    check(inp, want, counters, route, walk_level(route, inp.new_read_count) if level is None else level)
    return want


def _column_sets(text):
    cols = [l.split(b"\t") for l in text.split(b"\n")[:-1]]
    return [{c[k] for c in cols} for k in range(13)]


# ---- 1. one-field ladders (R1) ----------------------------------------------------------------------------------------------------
def case_ladder(field, pair, route):
    rows = T.ladder_rows(field, PAIRS[pair])
    want = check_copied(rows, route)
    cols = _column_sets(want)
    assert {(a, b) for a in b"+-" for b in b"+-"} == {(l.split(b"\t")[5][0], l.split(b"\t")[6][0]) for l in want.split(b"\n")[:-1]}
    k = {"id1": 0, "id2": 1, "pos1": 2, "pos2": 3, "ord_": 4, "perc": 7, "len1": 9, "len2": 10}[field]
    assert cols[k] == {str(x).encode() for x in T.LADDER_VALUES[field]} and all(len(cols[j]) == 1 for j in range(13) if j not in (k, 5, 6))


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("field", T.LADDER_FIELDS)
def test_one_field_ladders(field, pair):
    case_ladder(field, pair, None)


# ---- 2. straddles and tail bits (R1) ----------------------------------------------------------------------------------------------
def case_straddle(field, route):
    below, above = T.split_kinds(field, T.STRADDLE_VALUES[field])
    assert below and above, "the family must hold keys that differ only below the split and keys that differ only above it"
    want = check_copied(T.straddle_rows(field), route)
    assert want.count(b"\n") == len(set(T.STRADDLE_VALUES[field]))


def case_tail(route):
    want = check_copied(T.tail_rows(), route)
    cols = _column_sets(want)
    assert cols[11] == cols[12] == {b"p", b"s"} and len(cols[10]) == len(T.I32) and want.count(b"\n") == 4 * len(T.I32)


def test_key_of_the_test_orders_like_the_text():
    """The keys the straddle families are chosen by are the text's order: sorting by key is sorting the column's text + tab."""
    for field, values in T.STRADDLE_VALUES.items():
        vals = sorted(set(values), key=lambda x: T.field_key(field, x))
        assert vals == sorted(set(values), key=lambda x: str(x).encode() + b"\t")
    assert T.key_unsigned(10 ** 10 - 1, 10) < 2 ** 35 and T.key_signed(2 ** 31 - 1) < 2 ** 40 and T.key_unsigned(999, 3) < 2 ** 11


@pytest.mark.parametrize("field", list(T.SPLIT_BIT))
def test_straddles(field):
    case_straddle(field, None)


def test_tail_bits_and_repeats():
    case_tail(None)


# ---- 3. the product scenario (R1) -------------------------------------------------------------------------------------------------
def case_product(route, new_read_count=None):
    want = check_copied(T.product_rows(), route, new_read_count=new_read_count)
    assert want.count(b"\n") == 19440


def test_product_scenario():
    case_product(None)


# ---- 4. sparse ids through the walk (R2) ------------------------------------------------------------------------------------------
def _hot_ids(ids, text):
    """Those of `ids` that some line names, the one most lines name first."""
    count = {}
    for l in text.split(b"\n")[:-1]:
        for c in l.split(b"\t")[:2]:
            count[int(c)] = count.get(int(c), 0) + 1
    named = sorted((i for i in sorted(int(x) for x in ids) if i in count), key=lambda i: -count[i])
    assert named
    return named


def _pairs_apart_in_the_top_pass_only(text, new_read_count):
    """Whether two lines name pairs of ids (lo, hi) with one hi whose lo differ, and differ only in the bits the topmost pass of
    the walk's pair sort looks at: a sort that ends one pass early leaves such pairs in each other's runs."""
    m = T.pair_sort_shape(new_read_count)[2]
    seen = {}
    for l in text.split(b"\n")[:-1]:
        a, b = sorted(int(c) for c in l.split(b"\t")[:2])
        seen.setdefault((b, a & ((1 << m) - 1)), set()).add(a)
    return any(len(v) > 1 for v in seen.values())


def _names(text, label):
    return any(str(label).encode() in l.split(b"\t")[:2] for l in text.split(b"\n")[:-1])


def case_sparse_ids(olib, seed, flags, route):
    inp = T.fno1_scenario(seed, 60, 20, 300, with_extras=True, flags=flags)
    dense, counters = T.oracle_fno1(olib, inp)
    n = inp.new_read_count
    hot = _hot_ids(inp.srs["id"], dense)  # ids of super-reads: they are in a line only as one of a pair of new ids
    top = hot[0]
    # into [0, 2^31): id_bits = 31, the pair sort runs over all of its 62 bits, 2^31 - 1 is the hi of a pair, and the super-reads
    # most lines name get labels that agree in their low 25 bits, so that the sort's topmost pass (bits 56 - 61) decides between pairs
    f = T.labels(seed, n, 2 ** 31, forced=[x for x in T.FORCED_LABELS if x < 2 ** 31] + T.top_pass_family(2 ** 31, 24), hot=hot)
    want = T.relabel_text(dense, f, resort=True)
    assert f[top] == 2 ** 31 - 1 and _names(want, 2 ** 31 - 1) and _pairs_apart_in_the_top_pass_only(want, 2 ** 31)
    check(T.relabel(inp, f, 2 ** 31), want, counters, route, walk_level(route, 2 ** 31))
    # one more: 2 * id_bits = 64, the walk leaves the device; the same bytes
    check(T.relabel(inp, f, 2 ** 31 + 1), want, counters, route, walk_level(route, 2 ** 31 + 1))
    # into [0, 10^10): ten-digit ids in induced lines
    f = T.labels(seed, n, 10 ** 10, forced=T.FORCED_LABELS, hot=hot)
    want = T.relabel_text(dense, f, resort=True)
    assert set(T.FORCED_LABELS) <= set(f.values()) and _names(want, 10 ** 10 - 1)
    check(T.relabel(inp, f, 10 ** 10), want, counters, route, walk_level(route, 10 ** 10))


def case_pair_sort_width(olib, new_read_count, route):
    """2 * id_bits at a pass boundary of the 8-bit radix sort and just past it; the largest label is in use, as the hi of a pair, and
    the super-reads most lines name carry labels that only the sort's topmost pass tells apart."""
    inp = T.fno1_scenario(3, 60, 20, 300, with_extras=True)
    dense, counters = T.oracle_fno1(olib, inp)
    f = T.labels(3, inp.new_read_count, new_read_count, forced=[0] + T.top_pass_family(new_read_count, 12), hot=_hot_ids(inp.srs["id"], dense))
    want = T.relabel_text(dense, f, resort=True)
    assert _names(want, new_read_count - 1) and max(f.values()) == new_read_count - 1 and _pairs_apart_in_the_top_pass_only(want, new_read_count)
    check(T.relabel(inp, f, new_read_count), want, counters, route, walk_level(route, new_read_count))


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("seed", range(8))
def test_sparse_ids_through_the_walk(olib, seed, flags):
    case_sparse_ids(olib, seed, flags, None)


@pytest.mark.parametrize("new_read_count", PASS_BOUNDARIES)
def test_pair_sort_width(olib, new_read_count):
    case_pair_sort_width(olib, new_read_count, None)


# ---- 5. node_bits (the oracle directly, dense ids) --------------------------------------------------------------------------------
def case_node_bits(olib, n_nodes, route):
    small = T.fno1_scenario(7, 60, 20, 300, with_extras=True)
    touched = set(int(v) for v in small.graph_edges["v1"]) | set(int(v) for v in small.graph_edges["v2"])
    ends = sorted(touched & set(int(v) for v in small.clique_nodes))
    inp = T.spread_vertices(small, n_nodes, ends[0], ends[-1])
    assert len(inp.nodes) == n_nodes and {0, n_nodes - 1} <= set(int(v) for v in inp.clique_nodes)
    for v in (0, n_nodes - 1):
        assert ((inp.graph_edges["v1"] == v) | (inp.graph_edges["v2"] == v)).any()
    want, counters = T.oracle_fno1(olib, inp)
    assert counters["u2sr"] + counters["v2sr"] + counters["sr2sr"] > 0
    check(inp, want, counters, route, walk_level(route, inp.new_read_count))


@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_vertex_count_at_a_power_of_two(olib, n_nodes):
    case_node_bits(olib, n_nodes, None)


# ---- 6. the fall-back thresholds (R1) ---------------------------------------------------------------------------------------------
def _threshold_rows(id_=77, perc=50):
    rows = T.ladder_rows("pos1", T.LOW_PAIR)
    return rows + [T.row(id1=5, id2=id_, perc=perc), T.row(id1=id_, id2=7, perc=perc, p1=True, len2=3), T.row(id1=id_, id2=7, perc=perc, src="branching")]


def case_threshold_id(route):
    check_copied(_threshold_rows(id_=10 ** 10 - 1), route)  # new_read_count = 10^10: the second half on the device
    check_copied(_threshold_rows(id_=10 ** 10), route, level=0)


def case_threshold_perc(route):
    check_copied(_threshold_rows(perc=999), route)
    check_copied(_threshold_rows(perc=1000), route, level=0)


def test_largest_id_of_the_keys_and_the_first_beyond():
    case_threshold_id(None)


def test_largest_percentage_of_the_keys_and_the_first_beyond():
    case_threshold_perc(None)


# ---- 7. FNO=3 (R2, order kept) ----------------------------------------------------------------------------------------------------
def case_fno3(olib, seed, flags, route):
    inp = T.fno3_scenario(seed, flags=flags)
    dense, counters = T.oracle_fno3(olib, inp)
    top = _hot_ids(inp.srs["id"], dense)[0]
    f = T.labels(seed, len(inp.srs), 10 ** 10, forced=T.FORCED_LABELS, hot=[top])
    want = T.relabel_text(dense, f, resort=False)
    assert f[top] == 10 ** 10 - 1 and _names(want, 10 ** 10 - 1)
    check(T.relabel(inp, f, 10 ** 10), want, counters, route, 0 if route is None else 1, run=F.find_next_overlaps3)
    f[top] = 10 ** 10  # one id beyond the device's text: the host form writes the file
    want = T.relabel_text(dense, f, resort=False)
    check(T.relabel(inp, f, 10 ** 10 + 1), want, counters, route, 0, run=F.find_next_overlaps3)


@pytest.mark.parametrize("flags", [0, F.NO_INCLUSIONS])
@pytest.mark.parametrize("seed", range(8))
def test_fno3_sparse_ids(olib, seed, flags):
    case_fno3(olib, seed, flags, None)
