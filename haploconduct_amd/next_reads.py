"""The next iteration's read store from super-reads (include/hcsr.h: hc_sr_keep_device, hc_sr_set_next_reads, hc_sr_next_reads_fetch and
the host mirror hc_host_sr_next_reads): which super-reads survive process_cliques (reference src/SRBuilder.cpp:983-1001), Read::test_N_rate
(src/Read.h:214-234), the trivial super-reads (src/SRBuilder.cpp:1282-1372) and the numbering across the three groups.  Record view,
result type and the plumbing shared by EdgeScorer.sr_set_next_reads (device) and host_next_reads (the mirror)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .readstore import ReadSet

# hc_sr_next_entry, 32 bytes
NEXT_ENTRY_DTYPE = np.dtype([("off1", "<u8"), ("off2", "<u8"), ("len1", "<u4"), ("len2", "<u4"), ("read", "<u4"), ("kind", "u1"), ("src1", "u1"),
                             ("src2", "u1"), ("rev", "u1")], align=False)
assert NEXT_ENTRY_DTYPE.itemsize == 32
NEXT_SINGLE, NEXT_PAIRED, NEXT_TRIVIAL, NEXT_TRIVIAL_PAIRED = range(4)
SRC_CONSENSUS, SRC_BYTES = range(2)
NEXT_KEPT, NEXT_DROPPED_EMPTY, NEXT_DROPPED_N_RATE, NEXT_DROPPED_SHORT, NEXT_BAD_ENTRY = range(5)
NEXT_EMPTY = 1  # HC_SR_NEXT_EMPTY: the call's status when nothing is kept


@dataclass
class NextReads:
    new_id: np.ndarray  # int32 per entry: rank among the kept entries, or -1
    status: np.ndarray  # uint32 per entry: NEXT_*
    counts: dict        # hc_sr_next_counts
    empty: bool         # nothing was kept: the old store is in place (device) / reads is None (mirror)
    reads: ReadSet = None  # the mirror: the arrays one would pass to set_reads next


def single(off, length, src=SRC_CONSENSUS):
    return (off, 0, length, 0, 0, NEXT_SINGLE, src, 0, 0)


def paired(off1, len1, off2, len2, src1=SRC_CONSENSUS, src2=SRC_CONSENSUS):
    return (off1, off2, len1, len2, 0, NEXT_PAIRED, src1, src2, 0)


def trivial(read, rev=False, is_paired=False):
    return (0, 0, 0, 0, read, NEXT_TRIVIAL_PAIRED if is_paired else NEXT_TRIVIAL, 0, 0, int(rev))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _bytes(a):
    return np.ascontiguousarray(a if a is not None else np.zeros(0, np.uint8), dtype=np.uint8)


def _call_args(entries, extra_seq, extra_qual, keep_singletons):
    entries = np.ascontiguousarray(entries, dtype=NEXT_ENTRY_DTYPE)
    extra_seq, extra_qual = _bytes(extra_seq), _bytes(extra_qual)
    if extra_seq.size != extra_qual.size:
        raise ValueError("extra_seq and extra_qual differ in length")
    st = N.hc_sr_next_settings(int(keep_singletons), 0)
    new_id = np.full(entries.size, -1, np.int32)
    status = np.zeros(entries.size, np.uint32)
    counts = N.hc_sr_next_counts()
    keep = (entries, extra_seq, extra_qual, st)
    return keep, new_id, status, counts, [_ptr(entries), entries.size, _ptr(extra_seq), _ptr(extra_qual), extra_seq.size, C.byref(st), _ptr(new_id),
                                          _ptr(status), C.byref(counts)]


def set_next_reads(ctx, entries, extra_seq=None, extra_qual=None, keep_singletons=0):
    """hc_sr_set_next_reads on a context (EdgeScorer.sr_set_next_reads)."""
    keep, new_id, status, counts, args = _call_args(entries, extra_seq, extra_qual, keep_singletons)
    rc = N.lib.hc_sr_set_next_reads(ctx, *args)
    if rc not in (0, NEXT_EMPTY):
        N.check(rc, "hc_sr_set_next_reads")
    return NextReads(new_id, status, counts.as_dict(), rc == NEXT_EMPTY)


def fetch(ctx):
    """hc_sr_next_reads_fetch: the kept raw arrays of the context's store as a ReadSet (ids = the reads' indices)."""
    nb, ns, nr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = N.lib.hc_sr_next_reads_fetch(ctx, None, None, 0, None, None, 0, C.byref(nb), C.byref(ns), C.byref(nr))
    if rc != 0 and not (nb.value or ns.value or nr.value):
        N.check(rc, "hc_sr_next_reads_fetch")
    bases, quals = np.zeros(nb.value, np.uint8), np.zeros(nb.value, np.uint8)
    off, first = np.zeros(ns.value + 1, np.uint64), np.zeros(ns.value + 1, np.uint32)
    N.check(N.lib.hc_sr_next_reads_fetch(ctx, bases.ctypes.data, quals.ctypes.data, nb.value, off.ctypes.data, first.ctypes.data, ns.value,
                                         C.byref(nb), C.byref(ns), C.byref(nr)), "hc_sr_next_reads_fetch")
    return ReadSet(bases, quals, off, first[:nr.value + 1], np.arange(nr.value, dtype=np.uint64))


def host_next_reads(reads, cons_seq, cons_qual, entries, extra_seq=None, extra_qual=None, keep_singletons=0):
    """hc_host_sr_next_reads: the host mirror.  reads: the current ReadSet (may be None when no entry is a trivial)."""
    keep, new_id, status, counts, args = _call_args(entries, extra_seq, extra_qual, keep_singletons)
    cons_seq, cons_qual = _bytes(cons_seq), _bytes(cons_qual)
    if cons_seq.size != cons_qual.size:
        raise ValueError("cons_seq and cons_qual differ in length")
    n = keep[0].size
    store = [_ptr(reads.bases), _ptr(reads.quals), reads.seq_off.ctypes.data, reads.read_first_seq.ctypes.data, reads.n_reads] if reads is not None \
        else [None, None, None, None, 0]
    off, first = np.zeros(2 * n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    nb = C.c_uint64()

    def once(ob, oq, cap):
        return N.lib.hc_host_sr_next_reads(*store, _ptr(cons_seq), _ptr(cons_qual), cons_seq.size, *args, _ptr(ob), _ptr(oq), cap, C.byref(nb),
                                           off.ctypes.data, first.ctypes.data)

    rc = once(None, None, 0)  # count ...
    if rc == NEXT_EMPTY:
        return NextReads(new_id, status, counts.as_dict(), True)
    if rc != 0 and counts.n_kept == 0:
        N.check(rc, "hc_host_sr_next_reads")
    ob, oq = np.zeros(nb.value, np.uint8), np.zeros(nb.value, np.uint8)
    N.check(once(ob, oq, ob.size), "hc_host_sr_next_reads")  # ... then fetch
    nr, ns = int(counts.n_kept), int(counts.n_seq)
    return NextReads(new_id, status, counts.as_dict(), False, ReadSet(ob, oq, off[:ns + 1], first[:nr + 1], np.arange(nr, dtype=np.uint64)))
