"""Reference-guided overlaps enumerated on the device (hc_set_sam_records, hc_sam_plan, hc_sam_lines_device) against the host mirror, which
tests/test_sam_ingest.py pins to the reference's own scripts/sam2overlaps.py: the lines array for array, and the golden bytes after the
writer.  Every test asserts the device route: a plan that returned lines came from the device (there is no fall-back inside the context
calls), and the stage reports its route.  Hundreds of records each: shapes, not a workload."""
import json
import os

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import host
from haploconduct_amd.records import SAM_CIGAR_PLAIN, SAM_ID_PLAIN
from tests import _sam

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "sam", "cases.json")))
GOOD = sorted(k for k, c in CASES.items() if "expected" in c)
HC_ERR_NOT_ON_DEVICE = -11
COUNTERS = ("inclusion_count", "dup_count", "edges_added", "nonedges_written", "prefilter_rejected", "lines_read", "scored", "self_overlap_count",
            "silently_dropped")


@pytest.fixture(scope="module")
def sc():
    with hc.EdgeScorer(hc.Settings()) as s:
        yield s


def device_lines(sc, sam, mol, piece=None):
    sc.set_sam_records(sam)
    n = sc.sam_plan(mol)
    if piece is None:
        return sc.sam_lines(0, n)
    parts = [sc.sam_lines(at, min(piece, n - at)) for at in range(0, n, piece)]
    return np.concatenate(parts) if parts else sc.sam_lines(0, 0)


@pytest.mark.parametrize("name", GOOD)
def test_golden_cases(sc, name, tmp_path):
    case = CASES[name]
    sam = host.SamRecords.read(*_sam.write_inputs(case, tmp_path))
    if name == "text_ids":  # ids that are not plain decimals: the context call refuses, never a wrong line
        with pytest.raises(N.HcError) as e:
            sc.set_sam_records(sam)
        assert e.value.status == HC_ERR_NOT_ON_DEVICE
        return
    got = device_lines(sc, sam, case["min_overlap_len"])
    want, _ = sam.to_lines(case["min_overlap_len"])
    assert got.tobytes() == want.tobytes()
    out = str(tmp_path / "overlaps.txt")
    sam.write_lines(got, None, out)
    assert open(out, "rb").read() == case["expected"].encode()


SHAPES = {
    # all records at one position: the active set of the last record is every record in front of it
    "active_63": dict(seed=11, n_single=40, n_pair=24, same_pos=True),
    "active_64": dict(seed=12, n_single=40, n_pair=25, same_pos=True),
    "active_65": dict(seed=13, n_single=41, n_pair=25, same_pos=True),
    "active_300": dict(seed=14, n_single=200, n_pair=101, same_pos=True, max_ops=3),
    "mixed_lengths_with_holes": dict(seed=15, n_single=250, n_pair=150, lens=(60, 100, 150, 240), ref_len=(2500,)),
    "one_long_among_short": dict(seed=16, n_single=299, n_pair=0, lens=(100,), ref_len=(5000,), long_first=5000),
    "cigars_of_one_op": dict(seed=17, n_single=150, n_pair=100, ref_len=(1500,), max_ops=1),
    "cigars_of_nine_ops": dict(seed=18, n_single=150, n_pair=100, ref_len=(1500,), max_ops=9),
    "two_references": dict(seed=19, n_single=200, n_pair=150, lens=(80, 120), ref_len=(1500, 1100)),
    "past_the_references_end": dict(seed=20, n_single=100, n_pair=80, ref_len=(600,), span=900),
}


def make(shape):
    shape = dict(shape)
    long_first = shape.pop("long_first", None)
    sam = _sam.synth(**shape)
    if long_first:  # one read of `long_first` bases at the reference's start
        sam.alns["cpos"][0] = 1
        sam.alns["len"][0] = long_first
        sam.ops["count"][int(sam.alns["op_first"][0])] += long_first - 100
    return sam


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("mol", [0, 50])
def test_device_lines_equal_the_mirrors(sc, name, mol):
    sam = make(SHAPES[name])
    want, _ = sam.to_lines(mol)
    got = device_lines(sc, sam, mol)
    assert got.size == want.size and got.tobytes() == want.tobytes()
    assert want.size > 100
    cand, window = sc.sam_plan_counts()
    assert cand >= want.size and window >= cand
    if name.startswith("cigars_of"):
        assert int(sam.alns["op_count"].max()) == (1 if name.endswith("one_op") else 9)
    if name == "one_long_among_short":  # the device's while the windows hold at most 64 records per evaluated pair and record
        assert window <= 64 * (cand + sam.recs.size) and window > 4 * cand


def test_a_long_read_over_thousands_of_sparse_reads_is_refused(sc):
    """the windows reach back to the long read although almost nothing in them is active: quadratic, so the plan refuses"""
    sam = make(dict(seed=21, n_single=4000, n_pair=0, lens=(100,), ref_len=(2000000,), long_first=1999000, max_ops=1))
    sc.set_sam_records(sam)
    with pytest.raises(N.HcError) as e:
        sc.sam_plan(50)
    assert e.value.status == HC_ERR_NOT_ON_DEVICE
    cand, window = sc.sam_plan_counts()
    assert window > 64 * (cand + sam.recs.size)
    assert sam.to_lines(50)[0].size > 0  # the mirror's, by the host route


@pytest.mark.parametrize("piece", [1, 64, 1000])
def test_line_ranges_in_pieces(sc, piece):
    sam = make(SHAPES["mixed_lengths_with_holes"] if piece > 1 else SHAPES["active_65"])
    want, _ = sam.to_lines(20)
    got = device_lines(sc, sam, 20, piece=piece)
    assert got.tobytes() == want.tobytes() and want.size > max(piece, 100)
    with pytest.raises(N.HcError):
        sc.sam_lines(want.size, 1)  # beyond the file's end


def test_an_empty_result(sc):
    sam = _sam.synth(seed=22, n_single=200, n_pair=100, ref_len=(100000,), max_ops=1)  # sparse: no overlap longer than 100
    want, _ = sam.to_lines(100)
    assert want.size == 0
    sc.set_sam_records(sam)
    assert sc.sam_plan(100) == 0 and sc.sam_lines(0, 0).size == 0


def test_what_the_device_does_not_decide(sc):
    sam = _sam.synth(seed=23, n_single=20, n_pair=10)
    sam.alns["marks"][3] = SAM_CIGAR_PLAIN  # an id that is not a plain decimal
    with pytest.raises(N.HcError) as e:
        sc.set_sam_records(sam)
    assert e.value.status == HC_ERR_NOT_ON_DEVICE
    sam = _sam.synth(seed=23, n_single=20, n_pair=10)
    sam.alns["marks"][5] = SAM_ID_PLAIN  # `*`: no operation at all (the script's IndexError)
    sam.alns["op_count"][5] = 0
    with pytest.raises(N.HcError) as e:
        sc.set_sam_records(sam)
    assert e.value.status == HC_ERR_NOT_ON_DEVICE
    sam = _sam.synth(seed=23, n_single=20, n_pair=10)
    sam.alns["len"][int(sam.recs["second"][25])] = 0  # a second mate without a base: the script divides by its length
    with pytest.raises(N.HcError) as e:
        sc.set_sam_records(sam)
    assert e.value.status == HC_ERR_NOT_ON_DEVICE
    sam = _sam.synth(seed=23, n_single=20, n_pair=10, same_pos=True)
    sam.alns["len"][int(sam.recs["first"][2])] = 0  # ... and where only the count pass can see it (min_overlap_len < 0)
    sc.set_sam_records(sam)
    with pytest.raises(N.HcError) as e:
        sc.sam_plan(-1)
    assert e.value.status == HC_ERR_NOT_ON_DEVICE
    with pytest.raises(N.HcError) as e:
        sam.to_lines(-1)
    assert "ZeroDivisionError" in str(e.value)


# ---- the stage ----------------------------------------------------------------------------------------------------------------------
def stage_inputs(tmp_path, seed=31, n_single=120, n_pair=90, glen=900, L=80):
    """reads cut from one genome, written as FASTQ and as the SAM lines bwa would give them (forward strand, no clipping)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, glen)]

    def piece(s):
        seg = genome[s:s + L].copy()
        k = rng.random(L) < 0.004
        seg[k] = acgt[rng.integers(0, 4, int(k.sum()))]
        return seg.tobytes(), b"I" * L

    s_pos = [int(rng.integers(0, glen - L)) for _ in range(n_single)]
    p_pos = [(a, min(glen - L, a + int(rng.integers(10, 200)))) for a in (int(rng.integers(0, glen - L)) for _ in range(n_pair))]
    singles = [piece(s) for s in s_pos]
    pairs = [(piece(a), piece(b)) for a, b in p_pos]
    reads = hc.ReadSet.from_lists(singles, pairs)
    d = str(tmp_path) + "/"
    fq = dict(singles=d + "s.fastq", paired1=d + "p1.fastq", paired2=d + "p2.fastq")
    reads.write_fastq(fq["singles"], fq["paired1"], fq["paired2"])

    def line(rid, flag, pos, sq):
        return "\t".join([str(rid), str(flag), "g", str(pos + 1), "60", f"{L}M", "=", "0", "0", sq[0].decode(), sq[1].decode()]) + "\n"

    with open(d + "s.sam", "w") as f:
        f.write("@SQ\tSN:g\tLN:%d\n" % glen)
        for k, s in enumerate(s_pos):
            f.write(line(k, 0, s, singles[k]))
    with open(d + "p.sam", "w") as f:
        for k, (a, b) in enumerate(p_pos):
            f.write(line(n_single + k, 65, a, pairs[k][0]))
            f.write(line(n_single + k, 129, b, pairs[k][1]))
    with open(d + "ref.fasta", "w") as f:
        f.write(">g\n" + genome.tobytes().decode() + "\n")
    return fq, d + "s.sam", d + "p.sam", d + "ref.fasta"


def snapshot(ec, d):
    return ec.edges(), ec.in_lists(), ec.inclusions(), ec.counters(), open(os.path.join(d, "nonedge_overlaps.txt"), "rb").read()


@pytest.mark.parametrize("sorted_order,text_block", [(True, None), (False, None), (True, "4096")])
def test_stage_from_sam_equals_the_file_route(tmp_path, monkeypatch, sorted_order, text_block):
    if text_block:  # blocks of 186 lines, three in flight: the line ranges take turns in three of the context's slots
        monkeypatch.setenv("HC_TEXT_BLOCK", text_block)
        monkeypatch.setenv("HC_TEXT_DEPTH", "3")
    fq, sam_s, sam_p, ref = stage_inputs(tmp_path)
    st = hc.Settings(edge_threshold=0.9, ov_threshold=0.5, min_overlap_len=40)
    st.n_threads = 4
    mol = 30
    overlaps = str(tmp_path / "original_overlaps.txt")
    n_file = host.sam2overlaps(sam_s, sam_p, ref, overlaps, mol)
    assert n_file > 1000
    got = {}
    for route in ("device", "host", "file"):
        d = str(tmp_path / route) + "/"
        os.mkdir(d)
        with host.EdgeCalculatorStage(st, overlaps=overlaps if route == "file" else None, output_dir=d, **fq) as ec:
            if route == "file":
                ec.construct_edges_sorted() if sorted_order else ec.construct_edges()
            else:
                host.sam_on_device(route == "device")
                try:
                    n_rec, n_lines, on_device = ec.construct_edges_from_sam(sam_s, sam_p, ref, mol, sorted_order=sorted_order)
                finally:
                    host.sam_on_device(True)
                assert on_device == (route == "device"), "the route is not the one asked for"
                assert n_lines == n_file and n_rec == 210
            got[route] = snapshot(ec, d)
    want = got["file"]
    assert want[0].size > 200
    for route in ("device", "host"):
        a = got[route]
        assert a[0].size == want[0].size and a[0].tobytes() == want[0].tobytes(), f"{route}: the edges differ from the file route's"
        assert np.array_equal(a[1][0], want[1][0]) and np.array_equal(a[1][1], want[1][1]) and np.array_equal(a[2], want[2])
        for k in COUNTERS:
            assert a[3][k] == want[3][k], (route, k, a[3][k], want[3][k])
        assert a[4] == want[4], f"{route}: nonedge_overlaps.txt differs"
    assert got["device"][3]["host_blocks"] == 0 and got["device"][3]["host_lines"] == 0
    if text_block:
        assert got["device"][3]["device_blocks"] >= 6
