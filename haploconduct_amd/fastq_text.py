"""The FASTQ text of an iteration (include/hcsr.h: hc_sr_fastq_write_text, hc_sr_fastq_text_fetch and the host mirrors
hc_host_sr_fastq_text / hc_host_sr_fastq_tips_text): singles.fastq, paired1.fastq, paired2.fastq for a store's reads in ascending id and
removed_tip_sequences.fastq for the tips, as the reference's writers append them (src/SRBuilder.cpp:1386-1556).  Structure and the plumbing
shared by EdgeScorer.sr_fastq_text (device) and host.sr_fastq_text / host.sr_fastq_tips_text (the mirrors)."""
import ctypes as C

import numpy as np

from . import _native as N

_vp = C.c_void_p
_u64p = C.POINTER(C.c_uint64)

FASTQ_SINGLES, FASTQ_PAIRED1, FASTQ_PAIRED2, FASTQ_TIPS = range(4)  # HC_SR_FASTQ_*
FILES = ("singles", "paired1", "paired2", "tips")


class hc_sr_fastq_counts(C.Structure):
    _fields_ = [("n_records", C.c_uint64 * 4), ("n_bytes", C.c_uint64 * 4), ("ms_device", C.c_double)]


for _name, _args in (("hc_sr_fastq_write_text", [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(hc_sr_fastq_counts)]),
                     ("hc_sr_fastq_text_fetch", [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
                     ("hc_host_sr_fastq_text", [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _u64p]),
                     ("hc_host_sr_fastq_tips_text", [_vp, _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, _u64p])):
    getattr(N.lib, _name).restype = C.c_int
    getattr(N.lib, _name).argtypes = _args


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _u32(a):
    return np.ascontiguousarray(a if a is not None else np.zeros(0, np.uint32), dtype=np.uint32)


def write_text(ctx, tips=None, vertex_read=None):
    """hc_sr_fastq_write_text on a context -> hc_sr_fastq_counts; the text stays on the device (fetch)."""
    tips, vertex_read = _u32(tips), _u32(vertex_read)
    cn = hc_sr_fastq_counts()
    N.check(N.lib.hc_sr_fastq_write_text(ctx, _ptr(tips), tips.size, _ptr(vertex_read), vertex_read.size, C.byref(cn)), "hc_sr_fastq_write_text")
    return cn


def fetch(ctx, file, first, count):
    """hc_sr_fastq_text_fetch: bytes [first, first + count) of one file"""
    buf = np.zeros(int(count), np.uint8)
    N.check(N.lib.hc_sr_fastq_text_fetch(ctx, int(file), int(first), int(count), _ptr(buf)), "hc_sr_fastq_text_fetch")
    return buf.tobytes()


def text(ctx, tips=None, vertex_read=None):
    """write_text, then the four files whole (EdgeScorer.sr_fastq_text)."""
    cn = write_text(ctx, tips, vertex_read)
    out = {name: fetch(ctx, f, 0, cn.n_bytes[f]) for f, name in enumerate(FILES)}
    out["n_records"] = [int(x) for x in cn.n_records]
    out["n_bytes"] = [int(x) for x in cn.n_bytes]
    out["ms_device"] = float(cn.ms_device)
    return out


def _store(reads):
    return [_ptr(reads.bases), _ptr(reads.quals), reads.seq_off.ctypes.data, reads.read_first_seq.ctypes.data, reads.n_reads]


def _count_then_fetch(name, call):
    nb = C.c_uint64()
    rc = call(None, 0, C.byref(nb))  # count ...
    if rc != 0 and nb.value == 0:
        N.check(rc, name)
    buf = np.zeros(nb.value, np.uint8)
    if nb.value:
        N.check(call(_ptr(buf), buf.size, C.byref(nb)), name)  # ... then fetch
    return buf.tobytes()


def host_fastq_text(reads, file):
    """hc_host_sr_fastq_text: the bytes of singles.fastq (file 0), paired1.fastq (1) or paired2.fastq (2) for a ReadSet."""
    store = _store(reads)
    return _count_then_fetch("hc_host_sr_fastq_text", lambda p, cap, nb: N.lib.hc_host_sr_fastq_text(*store, int(file), p, cap, nb))


def host_fastq_tips_text(reads, tip_reads):
    """hc_host_sr_fastq_tips_text: the bytes of removed_tip_sequences.fastq for the reads tip_reads[k] of a ReadSet, k = the id."""
    store, tip_reads = _store(reads), _u32(tip_reads)
    return _count_then_fetch("hc_host_sr_fastq_tips_text",
                             lambda p, cap, nb: N.lib.hc_host_sr_fastq_tips_text(*store, _ptr(tip_reads), tip_reads.size, p, cap, nb))
