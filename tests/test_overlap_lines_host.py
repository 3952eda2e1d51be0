"""tests/_overlap_lines.py held against the host's readers — so that a wrong restatement cannot make the device's tests
(tests/test_gpu_text_reader.py) pass or fail for the wrong reason.  Over the corpus, the fuzz and the reference's own lines
(tests/golden/prefilter.json): the one-pass reader and the general path agree on every line, and every line the restatement calls plain
is accepted by both with the restatement's values.  No GPU needed."""
import json
import os

import pytest

from haploconduct_amd import host
from tests._overlap_lines import FIELDS, corpus, mutated, perc_of, plain_fields, split_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "prefilter.json")))


def _classes(lines):
    """(plain, accepted by the general path only, refused) after the checks of this file on every line."""
    n_plain = n_general = n_refused = 0
    for ln in lines:
        rc, o = host.parse_overlap(ln)
        rc2, o2 = host.parse_overlap(ln, general_only=True)
        assert rc == rc2 and o == o2, (ln, rc, rc2, o, o2)
        want = plain_fields(ln)
        if want is not None:
            assert rc == 0, ln
            got = dict(o, ord=ord(o["ord"]), ori1=ord(o["ori1"]), ori2=ord(o["ori2"]), type1=ord(o["type1"]), type2=ord(o["type2"]))
            for k in FIELDS:
                if k not in ("perc1", "perc2"):
                    assert got[k] == want[k], (ln, k)
            assert got["perc"] == perc_of(want), ln
            n_plain += 1
        elif rc == 0:
            n_general += 1
        else:
            n_refused += 1
    return n_plain, n_general, n_refused


def test_split_lines_is_getline():
    assert split_lines(b"") == [] and split_lines(b"\n") == [(0, 0)] and split_lines(b"x") == [(0, 1)]
    assert split_lines(b"ab\n\ncd") == [(0, 2), (3, 0), (4, 2)] and split_lines(b"ab\n\ncd\n") == [(0, 2), (3, 0), (4, 2)]
    assert split_lines(b"a\r\n\n") == [(0, 2), (3, 0)]


def test_the_restatement_on_lines_read_by_hand():
    ok = plain_fields(b"0\t999999999999999999\t007\t-\t-\t+\t-\t100\t101\t999999999\t5\ts\tp")
    assert ok == dict(id1=0, id2=10 ** 18 - 1, pos1=7, pos2=0, ord=45, ori1=43, ori2=45, perc1=100, perc2=0, len1=999999999, len2=0, type1=115, type2=112)
    assert perc_of(ok) == 100 and perc_of(dict(perc1=97, perc2=88)) == 92
    for bad in (b"01\t2\t0\t0\t1\t+\t+\t9\t9\t9\t9\tp\tp", b"1\t2\t0\t0\t1\t+\t+\t101\t9\t9\t9\tp\tp", b"1\t2\t0\t0\t-\t+\t+\t9\t9\t9\t9\tp\tp",
                b"1\t2\t0\t0\t1\t+\t+\t9\t9\t9\t9\ts\tp", b"1\t2\t0\t0\t1\t+\t+\t9\t9\t9\t9\tp\tp\t", b"1\t2\t0\t0\t1\t+\t+\t9\t9\t1234567890\t9\tp\tp",
                b"1\t2\t0\t0\t1\t+\t+\t9\t9\t9\t9\tp\tp\r", b"1\t2\t0\t0\t1\t*\t+\t9\t9\t9\t9\tp\tp", b"1" * 19 + b"\t2\t0\t0\t1\t+\t+\t9\t9\t9\t9\tp\tp"):
        assert plain_fields(bad) is None, bad


def test_corpus_against_both_host_readers():
    n_plain, n_general, n_refused = _classes(corpus())
    assert n_plain >= 50 and n_general >= 50 and n_refused >= 50, (n_plain, n_general, n_refused)


def test_fuzz_against_both_host_readers():
    n_plain, n_general, n_refused = _classes([ln.encode() for ln in mutated(17, 6000)])
    assert n_plain >= 2000 and n_general >= 1000 and n_refused >= 1500, (n_plain, n_general, n_refused)


def test_the_references_lines_against_both_host_readers():
    n_plain = 0
    for b in GOLD["blocks"]:
        lines = [ln.encode() for ln in b["lines"]]
        n_plain += _classes(lines)[0]
        assert not any(v == 3 and plain_fields(ln) is not None for ln, v in zip(lines, b["verdict"])), "a line the reference refuses is plain"
    assert n_plain >= 1700, n_plain
