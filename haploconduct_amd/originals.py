"""The original-read index maps (OverlapGraph::original_ID_dict, reference src/OverlapGraph.cpp:768-846) and subreads.txt (include/hcsr.h:
hc_sr_originals_* and the host mirrors hc_host_sr_originals_*): the dict of the next store from the dict of the current one and what
hc_sr_merge_next / hc_sr_clique_next returned (src/SRBuilder.cpp:750-806, :938-949, :1161-1216, :1312-1369), and the writers' text
(:1449-1463).  Structures, dtype and the plumbing shared by EdgeScorer.sr_originals_* (device) and host.sr_originals_* (the mirrors).  A
dict is a CSR over the reads of a store: off (uint64, n_reads + 1) and entries (ORIGINAL_DTYPE) in ascending original id inside a read."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .consensus import SR_LAYOUT_DTYPE
from .fno import FNO_READ_DTYPE, FNO_SUBREAD_DTYPE

_vp = C.c_void_p

ORIGINAL_DTYPE = np.dtype([("id", "<u4"), ("index1", "<i4"), ("index2", "<i4"), ("len1", "<u4"), ("len2", "<u4"), ("paired", "u1"), ("forward", "u1"),
                           ("pad", "u1", (2,))])
assert ORIGINAL_DTYPE.itemsize == 24

ORIG_OK, ORIG_EMPTY_SOURCE, ORIG_SEQ0_OF_PAIRED, ORIG_RANGE = range(4)  # HC_SR_ORIG_*
SOME_FAILED = 1                                                         # HC_SR_ORIG_SOME_FAILED


class hc_sr_originals_input(C.Structure):
    _fields_ = [("kind", _vp), ("new_id", _vp), ("overlap_pos", _vp), ("first_layout", _vp), ("n_cliques", C.c_uint64), ("layouts", _vp),
                ("sr_clique", _vp), ("subread_off", _vp), ("subreads", _vp), ("n_srs", C.c_uint64), ("vertex_state", _vp), ("nodes", _vp),
                ("vertex_read", _vp), ("vertex_fwd", _vp), ("n_vertices", C.c_uint64), ("new_read_count", C.c_uint64), ("first_it", C.c_uint32),
                ("reserved", C.c_uint32)]


class hc_sr_originals_output(C.Structure):
    _fields_ = [("orig_off", _vp), ("status", _vp), ("n_entries", C.c_uint64), ("n_failed", C.c_uint64), ("ms_device", C.c_double),
                ("ms_copy", C.c_double)]


class hc_sr_originals_text_counts(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("n_lines", C.c_uint64), ("ms_device", C.c_double)]


_u64p = C.POINTER(C.c_uint64)
for _name, _args in (("hc_sr_originals_init", [_vp]),
                     ("hc_sr_originals_load", [_vp, _vp, _vp, C.c_uint64]),
                     ("hc_sr_originals_fetch", [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p]),
                     ("hc_sr_originals_next", [_vp, C.POINTER(hc_sr_originals_input), C.POINTER(hc_sr_originals_output)]),
                     ("hc_sr_originals_write_text", [_vp, C.POINTER(hc_sr_originals_text_counts)]),
                     ("hc_sr_originals_text_fetch", [_vp, C.c_uint64, C.c_uint64, _vp]),
                     ("hc_host_sr_originals_next", [_vp, _vp, C.c_uint64, C.POINTER(hc_sr_originals_input), C.POINTER(hc_sr_originals_output), _vp,
                                                    C.c_uint64, C.c_uint32]),
                     ("hc_host_sr_originals_text", [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _u64p]),
                     ("hc_host_sr_originals_parse", [_vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p, _u64p])):
    getattr(N.lib, _name).restype = C.c_int
    getattr(N.lib, _name).argtypes = _args


@dataclass
class Tables:
    """hc_sr_originals_input as arrays: what hc_sr_merge_next or hc_sr_clique_next returned and took (tables_from builds one)."""
    kind: np.ndarray          # uint32 per clique / pair: merge_next.MN_*
    new_id: np.ndarray        # int32 per clique
    overlap_pos: np.ndarray   # int32 per clique
    first_layout: np.ndarray  # uint64, n_cliques + 1
    layouts: np.ndarray       # SR_LAYOUT_DTYPE
    sr_clique: np.ndarray     # uint32 per surviving super-read
    subread_off: np.ndarray   # uint64, n_srs + 1
    subreads: np.ndarray      # FNO_SUBREAD_DTYPE, ascending vertex inside a super-read
    vertex_state: np.ndarray  # uint32 per vertex: merge_next.MN_V_*
    nodes: np.ndarray         # FNO_READ_DTYPE per vertex
    vertex_read: np.ndarray   # uint32 per vertex
    vertex_fwd: np.ndarray    # uint8 per vertex
    new_read_count: int
    first_it: bool


def tables_from(res, merged, vertex_read, vertex_fwd, first_it):
    """res: a clique_next.CliqueNext or a merge_next.MergeNext; merged: the consensus.SrCliqueLayouts / SrEdgeLayouts it was built from."""
    clique = hasattr(res, "clique_kind")
    return Tables(res.clique_kind if clique else res.pair_kind, res.clique_new_id if clique else res.pair_new_id, res.overlap_pos, merged.first_layout,
                  merged.layouts, res.sr_clique if clique else res.sr_pair, res.subread_off, res.subreads, res.vertex_state, res.nodes, vertex_read,
                  vertex_fwd, res.new_read_count, first_it)


@dataclass
class OriginalsNext:
    off: np.ndarray      # uint64, new_read_count + 1: the new dict's offsets
    status: np.ndarray   # uint32 per new read: ORIG_*
    n_entries: int
    n_failed: int
    ms_device: float
    ms_copy: float
    entries: np.ndarray = None  # the mirror: the new dict's entries (device: EdgeScorer.sr_originals_fetch)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _dict(off, entries):
    off, entries = _c(off, np.uint64), _c(entries, ORIGINAL_DTYPE)
    if off.size == 0:
        off = np.zeros(1, np.uint64)
    if entries.size < int(off[-1]):
        raise ValueError("fewer entries than off names")
    return off, entries


def _prepare(t):
    a = dict(kind=_c(t.kind, np.uint32), new_id=_c(t.new_id, np.int32), overlap_pos=_c(t.overlap_pos, np.int32), first_layout=_c(t.first_layout, np.uint64),
             layouts=_c(t.layouts, SR_LAYOUT_DTYPE).reshape(-1), sr_clique=_c(t.sr_clique, np.uint32), subread_off=_c(t.subread_off, np.uint64),
             subreads=_c(t.subreads, FNO_SUBREAD_DTYPE).reshape(-1), vertex_state=_c(t.vertex_state, np.uint32), nodes=_c(t.nodes, FNO_READ_DTYPE),
             vertex_read=_c(t.vertex_read, np.uint32), vertex_fwd=_c(t.vertex_fwd, np.uint8))
    for k in ("first_layout", "subread_off"):
        if a[k].size == 0:
            a[k] = np.zeros(1, np.uint64)
    nc, ns, nv = a["kind"].size, a["sr_clique"].size, a["vertex_read"].size
    if a["new_id"].size != nc or a["overlap_pos"].size != nc or a["first_layout"].size != nc + 1 or a["subread_off"].size != ns + 1:
        raise ValueError("the per-clique / per-super-read arrays differ in length")
    if a["vertex_state"].size != nv or a["nodes"].size != nv or a["vertex_fwd"].size != nv:
        raise ValueError("the per-vertex arrays differ in length")
    if a["layouts"].size < int(a["first_layout"][-1]) or a["subreads"].size < int(a["subread_off"][-1]):
        raise ValueError("fewer layouts or subread rows than the offsets name")
    inp = hc_sr_originals_input()
    for k, v in a.items():
        setattr(inp, k, _ptr(v))
    inp.first_layout, inp.subread_off = a["first_layout"].ctypes.data, a["subread_off"].ctypes.data
    inp.n_cliques, inp.n_srs, inp.n_vertices, inp.new_read_count, inp.first_it = nc, ns, nv, int(t.new_read_count), int(bool(t.first_it))
    n_new = int(t.new_read_count)
    o = dict(orig_off=np.zeros(n_new + 1, np.uint64), status=np.zeros(n_new, np.uint32))
    out = hc_sr_originals_output(o["orig_off"].ctypes.data, o["status"].ctypes.data)
    return a, inp, o, out


def _result(o, out, entries=None):
    return OriginalsNext(o["orig_off"], o["status"], int(out.n_entries), int(out.n_failed), float(out.ms_device), float(out.ms_copy), entries)


def init(ctx):
    N.check(N.lib.hc_sr_originals_init(ctx), "hc_sr_originals_init")


def load(ctx, off, entries):
    off, entries = _dict(off, entries)
    N.check(N.lib.hc_sr_originals_load(ctx, off.ctypes.data, _ptr(entries), off.size - 1), "hc_sr_originals_load")


def fetch(ctx):
    """-> (off, entries) of the kept dict: count, then fetch"""
    nr, ne = C.c_uint64(), C.c_uint64()
    N.lib.hc_sr_originals_fetch(ctx, None, 0, None, 0, C.byref(nr), C.byref(ne))
    off, entries = np.zeros(nr.value + 1, np.uint64), np.zeros(ne.value, ORIGINAL_DTYPE)
    N.check(N.lib.hc_sr_originals_fetch(ctx, off.ctypes.data, nr.value, _ptr(entries), ne.value, C.byref(nr), C.byref(ne)), "hc_sr_originals_fetch")
    return off, entries


def next_dict(ctx, tables):
    """hc_sr_originals_next on a context (EdgeScorer.sr_originals_next)."""
    keep, inp, o, out = _prepare(tables)
    rc = N.lib.hc_sr_originals_next(ctx, C.byref(inp), C.byref(out))
    if rc not in (0, SOME_FAILED):
        N.check(rc, "hc_sr_originals_next")
    return _result(o, out)


def text(ctx):
    """hc_sr_originals_write_text, then the whole text -> (bytes, ms_device)"""
    cn = hc_sr_originals_text_counts()
    N.check(N.lib.hc_sr_originals_write_text(ctx, C.byref(cn)), "hc_sr_originals_write_text")
    buf = np.zeros(int(cn.n_bytes), np.uint8)
    N.check(N.lib.hc_sr_originals_text_fetch(ctx, 0, buf.size, _ptr(buf)), "hc_sr_originals_text_fetch")
    return buf.tobytes(), float(cn.ms_device)


def host_next(off, entries, tables, n_threads=1, cap=None):
    """hc_host_sr_originals_next: the mirror.  off / entries: the dict of the store the merge call found.  cap: room for the new dict's
    entries where the caller knows a bound (one call instead of count, then fetch)."""
    off, entries = _dict(off, entries)
    keep, inp, o, out = _prepare(tables)

    def once(dst, cap):
        return N.lib.hc_host_sr_originals_next(off.ctypes.data, _ptr(entries), off.size - 1, C.byref(inp), C.byref(out), _ptr(dst), cap, int(n_threads))

    if cap is None:
        rc = once(None, 0)  # count ...
        if rc not in (0, SOME_FAILED) and out.n_entries == 0:
            N.check(rc, "hc_host_sr_originals_next")
        cap = int(out.n_entries)
    dst = np.zeros(int(cap), ORIGINAL_DTYPE)
    rc = once(dst, dst.size)  # ... then fetch
    if rc not in (0, SOME_FAILED):
        N.check(rc, "hc_host_sr_originals_next")
    return _result(o, out, dst[:int(out.n_entries)])


def host_text(off, entries):
    off, entries = _dict(off, entries)
    nb = C.c_uint64()
    N.lib.hc_host_sr_originals_text(off.ctypes.data, _ptr(entries), off.size - 1, None, 0, C.byref(nb))
    buf = np.zeros(nb.value, np.uint8)
    N.check(N.lib.hc_host_sr_originals_text(off.ctypes.data, _ptr(entries), off.size - 1, _ptr(buf), buf.size, C.byref(nb)), "hc_host_sr_originals_text")
    return buf.tobytes()


def host_parse(data):
    """hc_host_sr_originals_parse: the bytes of a subreads.txt -> (off, entries).  HcError (HC_ERR_FORMAT) carries .line."""
    buf = np.frombuffer(bytes(data), np.uint8)
    nr, ne, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = N.lib.hc_host_sr_originals_parse(_ptr(buf), buf.size, None, 0, None, 0, C.byref(nr), C.byref(ne), C.byref(bad))
    if rc == -9:  # HC_ERR_FORMAT
        try:
            N.check(rc, "hc_host_sr_originals_parse")
        except Exception as e:
            e.line = int(bad.value)
            raise
    off, entries = np.zeros(nr.value + 1, np.uint64), np.zeros(ne.value, ORIGINAL_DTYPE)
    N.check(N.lib.hc_host_sr_originals_parse(_ptr(buf), buf.size, off.ctypes.data, nr.value, _ptr(entries), ne.value, C.byref(nr), C.byref(ne), C.byref(bad)),
            "hc_host_sr_originals_parse")
    return off, entries


# ---- FNO=3 from the kept dict: hc_fno3_from_originals and its mirror (include/hcsr.h) --------------------------------------------------
FNO3_CANDIDATE_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("original_id", "<u4"), ("flags", "<u4")])
assert FNO3_CANDIDATE_DTYPE.itemsize == 16
CAND_AMBIGUOUS, CAND_LINE = 1, 2  # HC_FNO3_CAND_*


class hc_fno3_resident_input(C.Structure):
    _fields_ = [("n_single", C.c_uint64), ("n_trivial", C.c_uint64), ("n_paired", C.c_uint64), ("walk_rank", _vp), ("original_readcount", C.c_uint64),
                ("max_combos", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class hc_fno3_resident_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_lines", "n_bytes", "candidates", "n_combos", "n_ambiguous", "n_originals")] + [("ms_device", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


for _name, _args in (("hc_fno3_from_originals", [_vp, C.POINTER(hc_fno3_resident_input), C.POINTER(hc_fno3_resident_counts)]),
                     ("hc_fno3_text_fetch", [_vp, C.c_uint64, C.c_uint64, _vp]),
                     ("hc_fno3_candidates_fetch", [_vp, C.c_uint64, C.c_uint64, _vp]),
                     ("hc_host_fno3_from_originals", [_vp, _vp, C.c_uint64, _vp, C.POINTER(hc_fno3_resident_input), C.POINTER(hc_fno3_resident_counts),
                                                      _vp, C.c_uint64, _u64p, _vp, C.c_uint64])):
    getattr(N.lib, _name).restype = C.c_int
    getattr(N.lib, _name).argtypes = _args


@dataclass
class Fno3Resident:
    text: bytes              # the lines, ascending (walk rank of SR1, walk rank of SR2)
    counts: dict             # hc_fno3_resident_counts
    candidates: np.ndarray   # FNO3_CANDIDATE_DTYPE, one per pair, in the order of the lines


def _fno3_input(counts3, walk_rank, original_readcount, max_combos, flags):
    inp = hc_fno3_resident_input()
    inp.n_single, inp.n_trivial, inp.n_paired = (int(x) for x in counts3)
    rank = None if walk_rank is None else _c(walk_rank, np.uint32)
    inp.walk_rank = None if rank is None else rank.ctypes.data
    inp.original_readcount, inp.max_combos, inp.flags = int(original_readcount), int(max_combos), int(flags)
    return inp, rank


def fno3_run(ctx, counts3, original_readcount, walk_rank=None, max_combos=0, flags=0):
    """hc_fno3_from_originals on a context; the text and the table stay on the device -> the counts as a dict."""
    inp, keep = _fno3_input(counts3, walk_rank, original_readcount, max_combos, flags)
    cn = hc_fno3_resident_counts()
    N.check(N.lib.hc_fno3_from_originals(ctx, C.byref(inp), C.byref(cn)), "hc_fno3_from_originals")
    return cn.as_dict()


def fno3_text(ctx, first, count):
    buf = np.zeros(int(count), np.uint8)
    N.check(N.lib.hc_fno3_text_fetch(ctx, int(first), buf.size, _ptr(buf)), "hc_fno3_text_fetch")
    return buf.tobytes()


def fno3_candidates(ctx, first, count):
    buf = np.zeros(int(count), FNO3_CANDIDATE_DTYPE)
    N.check(N.lib.hc_fno3_candidates_fetch(ctx, int(first), buf.size, _ptr(buf)), "hc_fno3_candidates_fetch")
    return buf


def fno3_from_originals(ctx, counts3, original_readcount, walk_rank=None, max_combos=0, flags=0):
    """The call, then the whole text and the whole table (EdgeScorer.fno3_from_originals) -> Fno3Resident."""
    cn = fno3_run(ctx, counts3, original_readcount, walk_rank, max_combos, flags)
    return Fno3Resident(fno3_text(ctx, 0, cn["n_bytes"]), cn, fno3_candidates(ctx, 0, cn["candidates"]))


def host_fno3_from_originals(off, entries, reads, counts3, original_readcount, walk_rank=None, max_combos=0, flags=0):
    """hc_host_fno3_from_originals: the mirror.  reads: FNO_READ_DTYPE per read of the dict (id: what the lines print) -> Fno3Resident."""
    off, entries = _dict(off, entries)
    reads = _c(reads, FNO_READ_DTYPE)
    if reads.size != off.size - 1:
        raise ValueError("one read per read of the dict")
    inp, keep = _fno3_input(counts3, walk_rank, original_readcount, max_combos, flags)
    cn, nb = hc_fno3_resident_counts(), C.c_uint64()

    def once(text, cands):
        return N.lib.hc_host_fno3_from_originals(off.ctypes.data, _ptr(entries), off.size - 1, _ptr(reads), C.byref(inp), C.byref(cn), _ptr(text),
                                                 text.size, C.byref(nb), _ptr(cands), cands.size)

    text, cands = np.zeros(0, np.uint8), np.zeros(0, FNO3_CANDIDATE_DTYPE)
    rc = once(text, cands)  # count ...
    if rc != 0 and not (rc == -1 and (cn.n_bytes or cn.candidates)):
        N.check(rc, "hc_host_fno3_from_originals")
    if rc != 0:
        text, cands = np.zeros(int(cn.n_bytes), np.uint8), np.zeros(int(cn.candidates), FNO3_CANDIDATE_DTYPE)
        N.check(once(text, cands), "hc_host_fno3_from_originals")  # ... then fetch
    return Fno3Resident(text.tobytes(), cn.as_dict(), cands)
