"""hc_host_sr_fastq_text / hc_host_sr_fastq_tips_text (include/hcsr.h), the host mirrors of the FASTQ writers: against the bytes the reference's
own writers left (tests/golden/fastq_text.json: src/SRBuilder.cpp:1386-1556 run in mergeAlongEdges' order), against a plain-Python restatement
of the cited lines on seeded stores, the count-then-fetch contract, the refusals, and a round trip through the project's FASTQ reader."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import haploconduct_amd as hc
from haploconduct_amd import _native as N
from haploconduct_amd import fastq_text as FQ
from haploconduct_amd import host as H
from tests import _fastq_text as T

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fastq_text.json")))["cases"]

LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200, 1023, 1024, 1025, 3000]


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_mirrors_reproduce_the_reference_writers_byte_for_byte(case):
    store = T.store_of_case(case)
    assert store.n_reads == case["new_read_count"]
    for f in range(3):
        assert H.sr_fastq_text(store, f) == case["files"][T.FILE_NAMES[f]].encode("ascii"), T.FILE_NAMES[f]
    # the tips are reads of the store the writers' caller walked: here a store of the tips themselves, in tips_vec order
    tips = T.store_of_case(case, ("tips",))
    assert H.sr_fastq_tips_text(tips, np.arange(tips.n_reads)) == case["files"][T.FILE_NAMES[3]].encode("ascii")


def test_the_fixture_covers_what_it_says():
    names = " ".join(c["name"] for c in GOLD)
    assert len(GOLD) >= 12 and "9 -> 10" in names and "99 -> 100" in names
    assert any(not c["files"]["paired1.fastq"] and c["files"]["singles.fastq"] for c in GOLD)
    assert any(not c["files"]["singles.fastq"] and c["files"]["paired1.fastq"] for c in GOLD)
    both = [c for c in GOLD if {"seq2" in r for r in c["reads"] if r["vec"] == "tips"} == {True, False}]  # tips of both kinds
    assert both and all("_2\n" in c["files"][T.FILE_NAMES[3]] for c in both)
    assert any(c["files"][T.FILE_NAMES[3]] == "" and c["reads"] for c in GOLD)
    assert any("@100\n" in c["files"]["paired1.fastq"] + c["files"]["singles.fastq"] for c in GOLD)


@pytest.mark.parametrize("kind", ["single", "paired", "mixed"])
@pytest.mark.parametrize("seed", [1, 2])
def test_mirrors_equal_the_restatement_on_seeded_stores(kind, seed):
    rng = np.random.default_rng(seed)
    lens = LENS + rng.integers(1, 300, 120).tolist()
    rng.shuffle(lens)
    store = T.make_store(rng, lens, kind)
    want = T.store_files(store)
    for f in range(3):
        assert H.sr_fastq_text(store, f) == want[f], f
    assert (want[0] == b"") == (kind == "paired") and (want[1] == b"") == (kind == "single")
    tips = rng.integers(0, store.n_reads, 25)  # (a read may be a tip twice: two vertices)
    assert H.sr_fastq_tips_text(store, tips) == T.tips_file(store, tips.tolist())
    assert H.sr_fastq_tips_text(store, []) == b""


def _raw_text(store, file, cap, with_buffer=True):
    nb = C.c_uint64(12345)
    buf = np.full(max(cap, 1), 0xAA, np.uint8)
    rc = N.lib.hc_host_sr_fastq_text(store.bases.ctypes.data, store.quals.ctypes.data, store.seq_off.ctypes.data, store.read_first_seq.ctypes.data,
                                     store.n_reads, file, buf.ctypes.data if with_buffer else None, cap, C.byref(nb))
    return rc, int(nb.value), buf


def _raw_tips(store, tips, cap, with_buffer=True):
    nb = C.c_uint64(12345)
    tips = np.ascontiguousarray(tips, np.uint32)
    buf = np.full(max(cap, 1), 0xAA, np.uint8)
    rc = N.lib.hc_host_sr_fastq_tips_text(store.bases.ctypes.data, store.quals.ctypes.data, store.seq_off.ctypes.data, store.read_first_seq.ctypes.data,
                                          store.n_reads, tips.ctypes.data, tips.size, buf.ctypes.data if with_buffer else None, cap, C.byref(nb))
    return rc, int(nb.value), buf


def test_count_then_fetch():
    store = T.make_store(np.random.default_rng(5), [20, 30, 40, 50, 60, 7], "mixed")
    for f in range(3):
        want = T.store_files(store)[f]
        assert want
        rc, nb, buf = _raw_text(store, f, 0, with_buffer=False)  # count
        assert rc == -1 and nb == len(want)
        rc, nb, buf = _raw_text(store, f, len(want) - 1)  # one byte short: nothing is copied
        assert rc == -1 and nb == len(want) and (buf == 0xAA).all()
        rc, nb, buf = _raw_text(store, f, len(want) + 3)  # room to spare: exactly n_bytes are written
        assert rc == 0 and nb == len(want) and buf[:nb].tobytes() == want and (buf[nb:] == 0xAA).all()
    tips = [0, 1, 2, 1]
    want = T.tips_file(store, tips)
    rc, nb, buf = _raw_tips(store, tips, 0, with_buffer=False)
    assert rc == -1 and nb == len(want)
    rc, nb, buf = _raw_tips(store, tips, len(want) - 1)
    assert rc == -1 and nb == len(want) and (buf == 0xAA).all()
    rc, nb, buf = _raw_tips(store, tips, len(want))
    assert rc == 0 and nb == len(want) and buf.tobytes() == want
    # nothing to write needs no buffer
    rc, nb, buf = _raw_tips(store, [], 0, with_buffer=False)
    assert rc == 0 and nb == 0


def test_refusals():
    store = T.make_store(np.random.default_rng(6), [20, 30, 40], "mixed")
    rc, nb, buf = _raw_tips(store, [0, store.n_reads], 10 ** 6)  # a tip read index >= n_reads
    assert rc == -1 and nb == 0 and (buf == 0xAA).all()
    with pytest.raises(hc.HcError, match="not below n_reads"):
        H.sr_fastq_tips_text(store, [store.n_reads])
    rc, nb, buf = _raw_text(store, 3, 10 ** 6)  # the tips are not a file of this call
    assert rc == -1 and nb == 0 and (buf == 0xAA).all()
    bad = np.array([0, 3, 4], np.uint32)  # a read of three sequences
    nbv = C.c_uint64()
    assert N.lib.hc_host_sr_fastq_text(store.bases.ctypes.data, store.quals.ctypes.data, store.seq_off.ctypes.data, bad.ctypes.data, 2, 0, None, 0, C.byref(nbv)) == -1
    assert N.lib.hc_host_sr_fastq_text(None, None, None, None, 0, 0, None, 0, C.byref(nbv)) == -1


def test_round_trip_through_the_fastq_reader(tmp_path, monkeypatch):
    """the mirror's three files read by host.Fastq (the reader tests/golden/fastq_pairs.json pins) give back the four raw arrays: a store with
    its single-end reads first, as the reader lays one out (src/FastqStorage.h:58-98)"""
    monkeypatch.setenv("HC_FASTQ_THREADS", "1")
    rng = np.random.default_rng(7)
    a, b = T.make_store(rng, LENS[:12] + [40, 50, 60], "single"), T.make_store(rng, LENS[:12] + [70, 80], "paired")
    store = hc.ReadSet(np.concatenate([a.bases, b.bases]), np.concatenate([a.quals, b.quals]),
                       np.concatenate([a.seq_off, b.seq_off[1:] + a.seq_off[-1]]),
                       np.concatenate([a.read_first_seq, b.read_first_seq[1:] + a.read_first_seq[-1]]), np.arange(a.n_reads + b.n_reads, dtype=np.uint64))
    paths = [str(tmp_path / n) for n in T.FILE_NAMES[:3]]
    for f, p in enumerate(paths):
        open(p, "wb").write(H.sr_fastq_text(store, f))
    back = H.Fastq(singles=paths[0], paired1=paths[1], paired2=paths[2], max_reads=100000)
    try:
        assert (back.n_single, back.n_paired) == (a.n_reads, b.n_reads)
        assert np.array_equal(back.bases, store.bases) and np.array_equal(back.quals, store.quals)
        assert np.array_equal(back.seq_off, store.seq_off) and np.array_equal(back.read_first_seq, store.read_first_seq)
        assert np.array_equal(back.read_ids, store.read_ids)
    finally:
        back.close()


def test_python_plumbing_names_the_files():
    assert FQ.FILES == ("singles", "paired1", "paired2", "tips") and (FQ.FASTQ_SINGLES, FQ.FASTQ_PAIRED1, FQ.FASTQ_PAIRED2, FQ.FASTQ_TIPS) == (0, 1, 2, 3)
