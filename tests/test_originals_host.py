"""hc_host_sr_originals_next / _text / _parse (include/hcsr.h), the host mirrors of the original-read index maps: against results recorded
from the reference's own statements (tests/golden/originals.json: constructSuperread's loop over the originals, merge_self_overlap's
shift, the trivials' reversal, the writers' lines and buildOriginalsDict's parse of them), against a plain-Python restatement of the cited
lines on seeded cases, parse(text(dict)) == dict, every status, and two-vertex cliques through the edge-merge and the clique input forms."""
import json
import os

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import host as H
from haploconduct_amd import merge_next as MN
from haploconduct_amd import originals as OR
from haploconduct_amd.consensus import SR_LAYOUT_DTYPE
from haploconduct_amd.fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE
from tests import _clique_next as Q
from tests import _merge_next as M
from tests import _originals as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "originals.json")

# seed, n_vertices, super-read sizes, keywords of _originals.make_case
SEEDED = [
    (1, 12, [2, 3], dict(first_it=True, dict_sizes=(1,))),
    (2, 40, [2, 3, 5, 8], dict()),
    (3, 40, [2, 3, 5, 8], dict(n_orig=12)),                              # a small pool: shared originals, the smallest vertex wins
    (4, 90, [40, 3, 2], dict(dict_sizes=(1, 2, 65), n_orig=400)),
    (5, 60, [2] * 12, dict(seq0=True)),
    (6, 60, [4] * 8, dict(seq0=True, first_it=True)),                    # first_it never reaches :801
    (7, 50, [3] * 6, dict(wide=True)),
    (8, 50, [3] * 6, dict(empty=0.3)),
    (9, 30, [10, 10], dict(share=True, dict_sizes=(5,))),
    (10, 1, [], dict()),
]


def _mirror_equals_restatement(maps, t, n_threads=1):
    off, entries = O.to_csr(maps)
    got = H.sr_originals_next(off, entries, t, n_threads=n_threads)
    want, status = O.next_restatement(maps, t)
    assert got.status.tolist() == status.tolist()
    O.assert_dict_equals_maps(got.off, got.entries, want, "next")
    assert got.n_failed == int((status != 0).sum()) and got.n_entries == got.entries.size == int(got.off[-1])
    return got, want, status


@pytest.mark.parametrize("k", range(len(SEEDED)))
def test_mirror_equals_the_restatement(k):
    seed, nv, sizes, kw = SEEDED[k]
    maps, t = O.make_case(seed, nv, sizes, **kw)
    got, want, _ = _mirror_equals_restatement(maps, t)
    # the text, and back
    text = H.sr_originals_text(got.off, got.entries)
    assert text == O.text_restatement(want)
    off2, entries2 = H.sr_originals_parse(text)
    assert off2.tolist() == got.off.tolist() and entries2.tobytes() == got.entries.tobytes()
    # threads change nothing
    again = H.sr_originals_next(*O.to_csr(maps), t, n_threads=5)
    assert again.off.tolist() == got.off.tolist() and again.entries.tobytes() == got.entries.tobytes() and again.status.tolist() == got.status.tolist()


def test_the_cases_hold_every_branch_and_status():
    seen, kinds, winners, negative = set(), set(), 0, 0
    for seed, nv, sizes, kw in SEEDED:
        maps, t = O.make_case(seed, nv, sizes, **kw)
        want, status = O.next_restatement(maps, t)
        seen |= set(status.tolist())
        kinds |= set(t.kind.tolist())
        for k, c in enumerate(t.sr_clique):
            ids = [oid for j in range(int(t.subread_off[k]), int(t.subread_off[k + 1])) for oid in maps[int(t.vertex_read[int(t.subreads[j]["node"])])]]
            winners += len(ids) != len(set(ids))
        negative += sum(e["index1"] < 0 for m in want if m for e in m.values())
    assert seen == {OR.ORIG_OK, OR.ORIG_EMPTY_SOURCE, OR.ORIG_SEQ0_OF_PAIRED, OR.ORIG_RANGE}
    assert kinds == set(range(6)) and winners > 5 and negative > 5


def test_a_status_is_decided_by_the_winners_only():
    """vertex 0 (forward) supplies original 7 first; vertex 1 (reverse, paired read) holds the same single-end original, which :762 skips
    before :801 is reached — and asserts when it comes first"""
    e = dict(index1=3, index2=0, len1=50, len2=0, paired=False, forward=True)
    maps = [{7: dict(e)}, {7: dict(e)}]
    nodes = np.zeros(2, FNO_READ_DTYPE)
    nodes["len1"], nodes["len2"], nodes["paired"] = (100, 100), (0, 90), (0, 1)

    def tables(order):
        subs = np.array([(v, 10, -1, 2, -1) for v in order], FNO_SUBREAD_DTYPE)
        return OR.Tables(np.array([MN.MN_SINGLE], np.uint32), np.array([0], np.int32), np.array([-1], np.int32), np.array([0, 1], np.uint64),
                         np.array([(0, 2, 150)], SR_LAYOUT_DTYPE), np.array([0], np.uint32), np.array([0, 2], np.uint64), subs,
                         np.zeros(2, np.uint32), nodes, np.array([0, 1], np.uint32), np.array([1, 0], np.uint8), 1, False)

    got, want, status = _mirror_equals_restatement(maps, tables([0, 1]))
    assert status.tolist() == [OR.ORIG_OK] and want[0][7]["index1"] == 3 + 8
    maps2 = [{7: dict(e)}, {7: dict(e), 9: dict(e)}]
    got, want, status = _mirror_equals_restatement(maps2, tables([0, 1]))
    assert status.tolist() == [OR.ORIG_SEQ0_OF_PAIRED] and got.n_entries == 0 and got.n_failed == 1  # original 9 wins under vertex 1


def test_range_and_the_priority_of_the_statuses():
    big = dict(index1=(1 << 31) - 5, index2=0, len1=50, len2=0, paired=False, forward=True)
    nodes = np.zeros(1, FNO_READ_DTYPE)
    nodes["len1"] = 100
    subs = np.array([(0, 10, -1, 0, -1)], FNO_SUBREAD_DTYPE)
    t = OR.Tables(np.array([MN.MN_SINGLE], np.uint32), np.array([0], np.int32), np.array([-1], np.int32), np.array([0, 1], np.uint64),
                  np.array([(0, 1, 150)], SR_LAYOUT_DTYPE), np.array([0], np.uint32), np.array([0, 1], np.uint64), subs, np.zeros(1, np.uint32), nodes,
                  np.array([0], np.uint32), np.array([1], np.uint8), 1, False)
    got, _, status = _mirror_equals_restatement([{4: big}], t)
    assert status.tolist() == [OR.ORIG_RANGE] and got.n_entries == 0
    small = dict(big, index1=(1 << 31) - 11)  # + 10 is the last int32
    got, _, status = _mirror_equals_restatement([{4: small}], t)
    assert status.tolist() == [OR.ORIG_OK] and got.entries["index1"][0] == (1 << 31) - 1


def test_two_vertex_cliques_give_the_same_dict_through_both_input_forms():
    c = Q.make_case(2, 64, [2] * 32, overlap=False)
    p = Q.as_pairs_case(c)
    a = Q.call_host(c, keep_singletons=8)
    b = M.call_host(p, keep_singletons=8)
    n = c.reads.n_reads
    paired = [c.reads.is_paired(r) for r in range(n)]
    first = c.reads.read_first_seq
    lens = np.diff(c.reads.seq_off.astype(np.int64))
    maps = O.first_it_restatement([lens[first[r]] for r in range(n)], [lens[first[r] + 1] if paired[r] else 0 for r in range(n)], paired)
    off, entries = O.to_csr(maps)
    for first_it in (True, False):
        ra = H.sr_originals_next(off, entries, a, c.merged, c.vertex_read, c.vertex_fwd, first_it=first_it)
        rb = H.sr_originals_next(off, entries, b, p.edge, p.vertex_read, p.vertex_fwd, first_it=first_it)
        assert ra.off.tolist() == rb.off.tolist() and ra.entries.tobytes() == rb.entries.tobytes() and ra.status.tolist() == rb.status.tolist()
        want, status = O.next_restatement(maps, OR.tables_from(a, c.merged, c.vertex_read, c.vertex_fwd, first_it))
        assert ra.status.tolist() == status.tolist()
        O.assert_dict_equals_maps(ra.off, ra.entries, want, "clique form")
        assert a.n_self_merged > 0 and ra.n_entries > 0


def test_parse_token_rules_and_statuses():
    off, entries = H.sr_originals_parse(b"0\t3:+:5:100\t2:-:-7,12:100,90\n2\t9::+,:1:5\n")
    assert off.tolist() == [0, 2, 2, 3]
    assert O.to_maps(off, entries) == [{2: dict(index1=-7, index2=12, len1=100, len2=90, paired=True, forward=False),
                                        3: dict(index1=5, index2=0, len1=100, len2=0, paired=False, forward=True)}, {},
                                       {9: dict(index1=1, index2=0, len1=5, len2=0, paired=False, forward=True)}]  # adjacent separators are one
    # the first line of an id and the first entry of an original stay (unordered_map::insert)
    off, entries = H.sr_originals_parse(b"1\t4:+:1:9\t4:-:2:9\n1\t5:+:1:9\n")
    assert O.to_maps(off, entries) == [{}, {4: dict(index1=1, index2=0, len1=9, len2=0, paired=False, forward=True)}]
    assert H.sr_originals_parse(b"")[0].tolist() == [0]
    assert H.sr_originals_parse(b"0\n")[0].tolist() == [0, 0]  # a read with no entry
    for bad, line in ((b"0\t3:+:5\n", 0), (b"0\t3:+:5:1\n1\t3:+:5,6:1\n", 1), (b"0\t3:+:5,6:1,2,3\n", 0), (b"0\t3:+:x:1\n", 0), (b"0\t\t3:+:5:1\n", 0),
                      (b"0\t3:+:5:1\nq\n", 1), (b"0\t3:+:99999999999:1\n", 0)):
        with pytest.raises(hc.HcError) as e:
            H.sr_originals_parse(bad)
        assert e.value.status == -9 and e.value.line == line, bad  # HC_ERR_FORMAT where the reference asserts (:816) or throws


def test_refusals():
    maps, t = O.make_case(2, 40, [2, 3, 5, 8])
    off, entries = O.to_csr(maps)
    for change, what in ((dict(new_read_count=3), "not below new_read_count"), (dict(vertex_read=t.vertex_read + 40), "no read of the kept dict"),
                         (dict(sr_clique=t.sr_clique + 9), "names no clique"), (dict(subread_off=t.subread_off[::-1].copy()), "subread_off")):
        bad = OR.Tables(**{**t.__dict__, **change})
        with pytest.raises(hc.HcError, match=what) as e:
            H.sr_originals_next(off, entries, bad)
        assert e.value.status == -1
    e2 = entries.copy()
    k = int(np.flatnonzero(np.diff(off.astype(np.int64)) >= 2)[0])
    e2["id"][int(off[k]) + 1] = e2["id"][int(off[k])]
    with pytest.raises(hc.HcError, match="strictly ascend"):
        H.sr_originals_next(off, e2, t)
    with pytest.raises(hc.HcError, match="descends"):
        H.sr_originals_text(np.array([0, 5, 3, int(off[-1])], np.uint64), entries)


def _golden():
    return json.load(open(GOLDEN))


def _golden_tables(case):
    a = case["tables"]
    nodes = np.zeros(len(a["nodes"]), FNO_READ_DTYPE)
    for v, (l1, l2, p) in enumerate(a["nodes"]):
        nodes[v]["len1"], nodes[v]["len2"], nodes[v]["paired"] = l1, l2, p
    for v, i in a["trivial_id"]:
        nodes[v]["id"] = i
    return OR.Tables(np.array(a["kind"], np.uint32), np.array(a["new_id"], np.int32), np.array(a["overlap_pos"], np.int32), np.array(a["first_layout"], np.uint64),
                     np.array([tuple(x) for x in a["layouts"]], SR_LAYOUT_DTYPE), np.array(a["sr_clique"], np.uint32), np.array(a["subread_off"], np.uint64),
                     np.array([tuple(x) for x in a["subreads"]], FNO_SUBREAD_DTYPE), np.array(a["vertex_state"], np.uint32), nodes,
                     np.array(a["vertex_read"], np.uint32), np.array(a["vertex_fwd"], np.uint8), a["new_read_count"], bool(a["first_it"]))


def _golden_maps(rows):
    """[[id, forward, index1, len1] | [id, forward, index1, len1, index2, len2], ...] per read -> maps"""
    return [{e[0]: dict(forward=bool(e[1]), index1=e[2], len1=e[3], paired=len(e) == 6, index2=e[4] if len(e) == 6 else 0, len2=e[5] if len(e) == 6 else 0)
             for e in m} for m in rows]


def test_mirrors_equal_the_recorded_reference_results():
    """every case of tests/golden/originals.json (tests/golden/make_golden_originals.py): the maps the reference's statements built, the lines
    its writer wrote — compared as the id plus the SET of fields, the order inside a line being libstdc++'s — and its parse of those lines"""
    doc = _golden()
    assert len(doc["cases"]) >= 12
    seen = set()
    for case in doc["cases"]:
        t = _golden_tables(case)
        maps = _golden_maps(case["dict"])
        off, entries = O.to_csr(maps)
        got = H.sr_originals_next(off, entries, t)
        assert not got.status.any(), case["name"]
        want = _golden_maps(case["want"])
        O.assert_dict_equals_maps(got.off, got.entries, want, case["name"])
        ours = H.sr_originals_text(got.off, got.entries).decode().split("\n")
        assert ours[-1] == "" and len(ours) - 1 == len(case["lines"])
        for mine, ref in zip(ours, case["lines"]):
            a, b = mine.split("\t"), ref.split("\t")
            assert a[0] == b[0] and sorted(a[1:]) == sorted(b[1:]) and len(a) == len(b), case["name"]
        # buildOriginalsDict's parse of the reference's own lines, and ours of the same bytes
        ref_text = "".join(l + "\n" for l in case["lines"]).encode()
        off2, entries2 = H.sr_originals_parse(ref_text)
        assert O.to_maps(off2, entries2) == [m or {} for m in want], case["name"]  # (the generator asserts the probe's parse == want)
        seen |= set(case["covers"])
    assert seen >= set(doc["required_cover"]), set(doc["required_cover"]) - seen
