"""The device's overlaps-text reader (csrc/hc_text_kernels.hip: text_count_kernel, text_scan_kernel, text_lines_kernel, text_parse_kernel with
parse_plain_line) pinned LINE BY LINE against the plain restatement of tests/_overlap_lines.py, which tests/test_overlap_lines_host.py holds
against the host's readers and the reference's own lines.  All comparisons are exact.  Three forms:
  the splitter alone   every line is junk, every line is listed (hc_textblock_list_nonplain): the list must be std::getline's lines;
  the grammar          a prefilter nothing passes: every plain line comes back as a reject with its parsed record, every other line listed;
  the reference's own  tests/golden/prefilter.json under each block's settings: listed / rejected / scored / dropped as the reference decided."""
import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd.records import LINE_DTYPE
from tests._overlap_lines import FIELDS, corpus, mutated, plain_fields, split_lines
from tests.test_prefilter_golden import GOLD, _settings

pytestmark = pytest.mark.gpu

# a prefilter nothing passes: 2 * LEN < 2^31 for every LEN of at most nine digits, --relax_PE_edges off (Settings' default flags)
NOTHING_PASSES = dict(min_overlap_len=1 << 31, min_overlap_perc=0)


def _scorer(**settings):
    sc = hc.EdgeScorer(hc.Settings(**settings))
    reads = hc.ReadSet.from_lists([("ACGTACGTAC" * 3, "I" * 30)] * 4)  # a tiny read set and its ids: the API wants both, nothing is scored
    sc.set_reads(reads)
    sc.set_ids(reads.read_ids)
    return sc


@pytest.fixture(scope="module")
def sc():
    with _scorer(**NOTHING_PASSES) as s:
        yield s


def _listed(b):
    return np.stack([b["nonplain"][k].astype(np.int64) for k in ("line_index", "begin", "length")], 1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------- the splitter alone
def _check_split(sc, text, routes=(False, True)):
    """One block of junk lines through hc_textblock_submit and the chained hc_textblock_submit_from: the listed lines are split_lines(text)."""
    want = split_lines(text)
    want_rows = np.array([(i, a, n) for i, (a, n) in enumerate(want)], np.int64).reshape(-1, 3)
    for chained in routes:
        blocks = sc.score_text(text, block_bytes=max(len(text), 64), max_bytes=max(len(text), 24 * len(want), 64), list_nonplain=True, chained=chained)
        assert len(blocks) == 1
        b = blocks[0]
        assert b["needs_host"] == 0, (len(text), chained)
        assert b["n_lines"] == b["n_nonplain"] == b["n_nonplain_listed"] == len(want), (len(text), chained, b["n_lines"], len(want))
        assert np.array_equal(_listed(b), want_rows), (len(text), chained)
        assert b["lines_read"] == len(want) and b["n_rejected"] == b["scored"] == b["self_overlaps"] == 0


def test_text_lengths_mod_16_behind_a_longer_text(sc):
    """(a) every text length mod 16, end closed and open, on a block that has just held a longer text of "x\\n" pairs: stale newlines lie
    behind the text's end, inside the last 16-byte piece and beyond."""
    P = 256
    stale = b"x\n" * (P // 2)  # 128 lines: more than a block of 1 024 bytes has room for (1024 / 24 + 16 = 58)
    seen = set()
    for L in list(range(1, 18)) + list(range(31, 49)):
        for closed in (True, False):
            t = (b"xxxxx\n" * 9)[: L - 1] + (b"\n" if closed else b"x")
            assert len(t) == L
            want = split_lines(t)
            want_rows = np.array([(i, a, n) for i, (a, n) in enumerate(want)], np.int64).reshape(-1, 3)
            for chained in (False, True):
                # blocks of P bytes: the stale text twice (chained submits alternate between two block objects), then the text under test
                out = sc.score_text(stale + stale + t, block_bytes=P, max_bytes=1024, list_nonplain=True, chained=chained)
                assert len(out) == 3 and out[2]["bytes"] == (2 * P, 2 * P + L)
                assert out[0]["needs_host"] == 1 and out[0]["n_lines"] == P // 2 > out[0]["max_lines"], "the earlier text is meant to have more lines than room"
                assert out[1]["needs_host"] == 1
                b = out[2]
                assert b["needs_host"] == 0 and b["n_lines"] == b["n_nonplain"] == len(want), (L, closed, chained, b["n_lines"], len(want))
                assert np.array_equal(_listed(b), want_rows), (L, closed, chained)
            seen.add((L % 16, closed))
    assert seen == {(r, c) for r in range(16) for c in (True, False)}


def _newline_offsets(text):
    return np.nonzero(np.frombuffer(text, np.uint8) == 10)[0]


def test_line_lengths(sc):
    """(b) a newline on every byte of a 16-byte piece, around a 4 KiB tile's edge, a tile without a newline, runs of newlines, the
    smallest texts."""
    every_offset = b"".join(b"x" * k + b"\n" for k in range(17)) * 2
    assert set((_newline_offsets(every_offset) % 16).tolist()) == set(range(16))
    tile_edge = b"x" * 4095 + b"\n\n\n" + b"x" * 10 + b"\n"
    assert _newline_offsets(tile_edge)[:3].tolist() == [4095, 4096, 4097]
    tile_lines = b"".join(b"x" * k + b"\n" for k in (4095, 4096, 4097))
    long_line = (b"x" * 99 + b"\n") * 40 + b"x" * 5000 + b"\n" + b"xx\n"
    assert not ((_newline_offsets(long_line) // 4096) == 1).any(), "the second tile is meant to hold no newline"
    runs = b"x\n\nxx\n\n\nx" + b"\n" * 17 + b"x\n"
    for text in (every_offset, every_offset[:-1], tile_edge, tile_edge[:4096], tile_edge[:4097], tile_lines, tile_lines[:-1], long_line, runs,
                 runs[:-2], b"\n", b"x", b""):
        _check_split(sc, text)


def test_a_text_of_more_than_1024_tiles(sc):
    """(c) 4.5 MiB of lines of about 100 bytes: 1 152 tiles, the scan's second round."""
    lengths = 90 + (np.arange(50000) * 7) % 21
    text = b"".join(b"x" * int(k) + b"\n" for k in lengths)[: 9 << 19]
    assert len(text) == 9 << 19 and (len(text) + 4095) // 4096 > 1024
    _check_split(sc, text)


@pytest.mark.parametrize("max_bytes", [64, 24000])
def test_exactly_as_many_lines_as_room(sc, max_bytes):
    """(d) max_lines lines with the end closed, with the end open (line_start[max_lines] is the scan kernel's to write), and one more."""
    m = sc.score_text(b"x", max_bytes=max_bytes, list_nonplain=True)[0]["max_lines"]
    assert 2 * (m + 1) <= max_bytes
    for text in (b"x\n" * m, b"x\n" * (m - 1) + b"x"):
        want = np.array([(i, 2 * i, 1) for i in range(m)], np.int64)
        for chained in (False, True):
            b = sc.score_text(text, block_bytes=max_bytes, max_bytes=max_bytes, list_nonplain=True, chained=chained)[0]
            assert b["needs_host"] == 0 and b["n_lines"] == b["n_nonplain"] == m, (len(text), chained, b["n_lines"])
            assert np.array_equal(_listed(b), want), (len(text), chained)
    for text in (b"x\n" * (m + 1), b"x\n" * m + b"x"):
        for chained in (False, True):
            b = sc.score_text(text, block_bytes=max_bytes, max_bytes=max_bytes, list_nonplain=True, chained=chained)[0]
            assert b["needs_host"] == 1 and b["n_lines"] == m + 1, (len(text), chained)


# ------------------------------------------------------------------------------------------------------------------ the grammar
def _expected(lines, below=None):
    """What a block of `lines` (bytes, joined by newlines) must give under NOTHING_PASSES, for the lines numbered < below:
    (listed rows, reject line numbers, reject records, number of self overlaps)."""
    listed, rej_at, rej, n_self, at = [], [], [], 0, 0
    for i, ln in enumerate(lines):
        if below is None or i < below:
            f = plain_fields(ln)
            if f is None:
                listed.append((i, at, len(ln)))
            elif f["id1"] == f["id2"]:
                n_self += 1
            else:
                rej_at.append(i)
                rej.append(tuple(f[k] for k in FIELDS))
        at += len(ln) + 1
    return np.array(listed, np.int64).reshape(-1, 3), rej_at, rej, n_self


def _check_grammar(b, lines, below=None, what=""):
    listed, rej_at, rej, n_self = _expected(lines, below)
    assert b["needs_host"] == 0 and b["n_lines"] == len(lines), what
    assert b["lines_read"] == (len(lines) if below is None else min(below, len(lines))), what
    got = _listed(b)
    assert got.shape == listed.shape and np.array_equal(got, listed), (what, "listed lines", got[:5], listed[:5])
    assert b["n_nonplain"] == len(listed)
    r = b["rejected"]
    assert r["line_index"].tolist() == rej_at and b["prefilter_rejected"] == b["n_rejected"] == len(rej_at), (what, "which lines are rejects")
    for j, k in enumerate(FIELDS):
        want = np.array([t[j] for t in rej], dtype=LINE_DTYPE.fields[k][0])
        assert np.array_equal(r["line"][k], want), (what, k)
    assert not r["line"]["pad"].any() and not r["pad"].any()
    assert b["self_overlaps"] == n_self and b["scored"] == b["silently_dropped"] == b["n_rows"] == 0, what


def _text(lines):
    assert not any(b"\n" in ln for ln in lines)
    return b"\n".join(lines) + b"\n"


def _one_block(sc, lines, chained=False, **kw):
    text = _text(lines)
    out = sc.score_text(text, block_bytes=len(text), max_bytes=max(len(text), 24 * len(lines), 64), list_nonplain=True, chained=chained, **kw)
    assert len(out) == 1
    return out[0]


def test_corpus_at_every_alignment(sc):
    """(e) the corpus behind a junk line of 0, 1, 2 and 3 bytes: every line at every alignment of the cursor's 4-byte window."""
    base = corpus()
    begins = []
    for j in range(4):
        lines = [b"x" * j] + base
        begins.append(np.array([a for a, _ in split_lines(_text(lines))[1:]]) % 4)
        for chained in (False, True):
            _check_grammar(_one_block(sc, lines, chained), lines, what=(j, chained))
    assert (np.sort(np.stack(begins), 0) == np.arange(4)[:, None]).all()


def test_corpus_through_the_unstaged_cursor(sc):
    """(f) a 40 000-byte junk line after every 128 lines: no aligned group of 256 lines fits the 32 KiB LDS window, every workgroup reads
    its lines from the block's text (Cursor<false>)."""
    lines = []
    for ln in [x for j in range(4) for x in [b"x" * j] + corpus()]:
        lines.append(ln)
        if len(lines) % 128 == 127:
            lines.append(b"x" * 40000)
    start = [a for a, _ in split_lines(_text(lines))] + [len(_text(lines))]
    for first in range(0, len(lines), 256):
        last = min(first + 256, len(lines))
        assert start[last] - start[first] > 32768, (first, last)
    for chained in (False, True):
        _check_grammar(_one_block(sc, lines, chained), lines, what=chained)


def test_fuzz(sc):
    """(g) mutated(17, 6000) as one text."""
    lines = [ln.encode() for ln in mutated(17, 6000)]
    b = _one_block(sc, lines)
    _check_grammar(b, lines)
    assert b["n_rejected"] >= 2000 and b["n_nonplain"] >= 2500


def test_more_rejects_than_room(sc):
    """(h) 20 000 plain lines, all rejects, in a block created just large enough: the reject buffer (an eighth of the lines + 4 096)
    overflows, the block grows it and runs its device half again — same records, and the list of lines that are not plain as it was."""
    lines = []
    for i in range(20000):
        lines.append(b"%d\t%d\t%d\t-\t-\t+\t-\t%d\t-\t%d\t-\ts\tp" % (i + 1, 3 * i + 2, i % 300, i % 101, 100 + i % 57))
        if i % 1000 == 500:
            lines.append(b"x" * (i // 1000))
    text = _text(lines)
    out = sc.score_text(text, block_bytes=len(text), list_nonplain=True)
    assert len(out) == 1 and 20000 > out[0]["max_lines"] // 8 + 4096
    assert out[0]["regrown"] >= 1
    _check_grammar(out[0], lines)
    assert out[0]["n_rejected"] == 20000 and out[0]["n_nonplain"] == 20


@pytest.mark.parametrize("first_line_no", [0, 1000])
def test_max_ov_cuts(first_line_no):
    """(i) --max_ov cutting the block at line 0, 1, 255, 256, 257, n - 1, n and n + 1: lines_read, and rejects and listed lines below the cut only."""
    lines = corpus() * 2
    n = len(lines)
    assert n > 257
    for cut in (0, 1, 255, 256, 257, n - 1, n, n + 1):
        with _scorer(max_overlaps=first_line_no + cut, **NOTHING_PASSES) as s:
            b = _one_block(s, lines, first_line_no=first_line_no)
        _check_grammar(b, lines, below=cut, what=(first_line_no, cut))


# -------------------------------------------------------------------------------------------------------- the reference's own lines
@pytest.fixture(scope="module")
def golden_reads():
    return hc.ReadSet.from_lists([("ACGTACGTAC" * 30, "I" * 300)] * 2200)  # every id the vectors name (tests/test_prefilter_golden.py)


@pytest.mark.parametrize("k", range(len(GOLD["blocks"])))
def test_the_references_lines(k, golden_reads):
    """Every line of tests/golden/prefilter.json under its block's settings: the device lists exactly the lines that are not plain — every
    line the reference refused among them — and decides the plain ones as the reference did."""
    g = GOLD["blocks"][k]
    lines = [ln.encode() for ln in g["lines"]]
    verdict = g["verdict"]
    with hc.EdgeScorer(_settings(g)) as s:
        s.set_reads(golden_reads)
        s.set_ids(golden_reads.read_ids)
        b = _one_block(s, lines)
    assert b["needs_host"] == 0 and b["n_lines"] == b["lines_read"] == len(lines)
    parsed = [plain_fields(ln) for ln in lines]
    start = [a for a, _ in split_lines(_text(lines))]
    want = np.array([(i, start[i], len(lines[i])) for i, f in enumerate(parsed) if f is None], np.int64).reshape(-1, 3)
    assert np.array_equal(_listed(b), want)
    assert {i for i, v in enumerate(verdict) if v == 3} <= set(want[:, 0].tolist())
    rej_at = [i for i, (f, v) in enumerate(zip(parsed, verdict)) if f is not None and v == 2]
    assert b["rejected"]["line_index"].tolist() == rej_at
    for kf in FIELDS:
        assert b["rejected"]["line"][kf].tolist() == [parsed[i][kf] for i in rej_at], kf
    assert b["scored"] == sum(1 for f, v in zip(parsed, verdict) if f is not None and v == 1)
    assert b["self_overlaps"] + b["silently_dropped"] == sum(1 for f, v in zip(parsed, verdict) if f is not None and v == 0)
    assert not any(f is not None and v == 3 for f, v in zip(parsed, verdict))
