"""The FASTQ files' text read on the device into the read store (include/hcedge.h: hc_set_reads_from_fastq_text, hc_fastq_fetch,
hc_fastq_set_chunk_bytes): the structures and the plumbing behind EdgeScorer.set_reads_from_fastq / .fastq_fetch / .fastq_set_chunk_bytes.
The call equals host.Fastq followed by set_reads on files holding the same bytes; `plain_id` restates which header tokens the device
reads itself (every other one is resolved by the host inside the call: hc_fastq_counts.n_host_ids)."""
import ctypes as C
import mmap
import os
import re

import numpy as np

from . import _native as N

_vp = C.c_void_p


class hc_fastq_text(C.Structure):
    _fields_ = [("singles", _vp), ("n_singles", C.c_uint64), ("paired1", _vp), ("n_paired1", C.c_uint64), ("paired2", _vp), ("n_paired2", C.c_uint64),
                ("ids_path", C.c_char_p), ("max_reads", C.c_uint64)]


class hc_fastq_counts(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_seq", C.c_uint32), ("n_single", C.c_uint32), ("n_paired", C.c_uint32), ("n_bytes", C.c_uint64),
                ("n_host_ids", C.c_uint64), ("err_record", C.c_uint64), ("err_file", C.c_int32), ("reserved", C.c_uint32), ("ms_copy", C.c_double),
                ("ms_device", C.c_double), ("ms_plan", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


for _name, _args in (("hc_set_reads_from_fastq_text", [_vp, C.POINTER(hc_fastq_text), C.POINTER(hc_fastq_counts)]),
                     ("hc_fastq_fetch", [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64]),
                     ("hc_fastq_set_chunk_bytes", [_vp, C.c_uint64])):
    getattr(N.lib, _name).restype = C.c_int
    getattr(N.lib, _name).argtypes = _args

DEFAULT_MAX_READS = 100000000  # program_settings.max_reads (host.make_paths: 0 = the default)

# parse_id's fast path, the tokens the device reads itself: 0 or [1-9][0-9]{0,17}
PLAIN_ID = re.compile(rb"0|[1-9][0-9]{0,17}")
_SPACE = b" \t\n\v\f\r"  # isspace in the C locale


def header_token(line):
    """`stream >> id` on a header line (bytes, without its newline) less its first character: the first run of non-space bytes."""
    rest = line[1:].lstrip(_SPACE)
    for i, b in enumerate(rest):
        if b in _SPACE:
            return rest[:i]
    return rest


def plain_id(token):
    return PLAIN_ID.fullmatch(token) is not None


def count_host_ids(text, max_reads=DEFAULT_MAX_READS):
    """How many of a file's records (bytes; every fourth line of at most 4 * max_reads, an incomplete last record ignored) have a header
    token that is not plain: hc_fastq_counts.n_host_ids of a call without an --IDs file."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # nothing behind a trailing newline
    n = min(len(lines), 4 * (max_reads & 0xFFFFFFFF)) // 4
    return sum(not plain_id(header_token(lines[4 * r])) for r in range(n))


class _Text:
    """The bytes of one file for the call: bytes as they are, or a read-only mapping of a path; None: no such file."""

    def __init__(self, src):
        self._map = self._file = self._keep = None
        self.ptr, self.n = None, 0
        if src is None:
            return
        if isinstance(src, (bytes, bytearray, memoryview)):
            self._keep = np.frombuffer(bytes(src), np.uint8)
        else:
            self._file = open(os.fspath(src), "rb")
            if os.fstat(self._file.fileno()).st_size:
                self._map = mmap.mmap(self._file.fileno(), 0, access=mmap.ACCESS_READ)
                self._keep = np.frombuffer(self._map, np.uint8)
            else:
                self._keep = np.zeros(0, np.uint8)
        self.n = int(self._keep.size)
        self._pad = np.zeros(1, np.uint8)
        self.ptr = self._keep.ctypes.data if self.n else self._pad.ctypes.data  # (an empty file is still a file)

    def close(self):
        self._keep = None
        if self._map is not None:
            self._map.close()
        if self._file is not None:
            self._file.close()


def set_reads_from_fastq(ctx, singles=None, paired1=None, paired2=None, ids=None, max_reads=0):
    """hc_set_reads_from_fastq_text on a context; singles / paired1 / paired2 are paths or bytes, ids the --IDs file's path.  Returns the
    hc_fastq_counts; a failure raises HcError with the counts (err_file, err_record) in its .counts."""
    texts = [_Text(singles), _Text(paired1), _Text(paired2)]
    try:
        tx = hc_fastq_text(texts[0].ptr, texts[0].n, texts[1].ptr, texts[1].n, texts[2].ptr, texts[2].n,
                           os.fsencode(ids) if ids is not None else None, int(max_reads) if max_reads else DEFAULT_MAX_READS)
        cn = hc_fastq_counts()
        rc = N.lib.hc_set_reads_from_fastq_text(ctx, C.byref(tx), C.byref(cn))
        if rc != 0:
            e = N.HcError(rc, "hc_set_reads_from_fastq_text")
            e.counts = cn
            raise e
        return cn
    finally:
        for t in texts:
            t.close()


def fetch(ctx, counts):
    """hc_fastq_fetch for the counts of the last call: (read_ids, seq_off, read_first_seq)."""
    read_ids = np.zeros(counts.n_reads, np.uint64)
    seq_off = np.zeros(counts.n_seq + 1, np.uint64)
    first = np.zeros(counts.n_reads + 1, np.uint32)
    N.check(N.lib.hc_fastq_fetch(ctx, read_ids.ctypes.data, read_ids.size, seq_off.ctypes.data, first.ctypes.data, counts.n_seq), "hc_fastq_fetch")
    return read_ids, seq_off, first


def set_chunk_bytes(ctx, n_bytes):
    N.check(N.lib.hc_fastq_set_chunk_bytes(ctx, int(n_bytes)), "hc_fastq_set_chunk_bytes")
