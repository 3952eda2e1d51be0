"""Super-read consensus (include/hcsr.h): SRBuilder::consensus / consensus_pos (reference src/SRBuilder.cpp:289-535)
for a batch of layouts.  Record views, the result type and the plumbing shared by EdgeScorer.sr_consensus (device)
and host.sr_consensus (the host mirror); the same for the merge of self-overlapping paired super-reads
(SRBuilder::merge_self_overlap, src/SRBuilder.cpp:872-955): EdgeScorer.sr_merge_self_overlaps / host.sr_merge_self_overlaps, and
EdgeScorer.sr_merge_self_overlaps_kept, which reads its mates from the consensus bytes kept on the device and appends to them."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N

# hc_sr_member, 12 bytes; hc_sr_layout, 16 bytes
SR_MEMBER_DTYPE = np.dtype([("read", "<u4"), ("pos", "<i4"), ("seq", "u1"), ("rev", "u1"), ("pad", "u1", (2,))], align=False)
assert SR_MEMBER_DTYPE.itemsize == 12
SR_LAYOUT_DTYPE = np.dtype([("first_member", "<u8"), ("n_members", "<u4"), ("total_len", "<i4")], align=False)
assert SR_LAYOUT_DTYPE.itemsize == 16

SR_OK, SR_NO_SUPPORT, SR_MEMBER_SHORT, SR_UNCOVERED, SR_NAN, SR_BAD_LAYOUT, SR_BAD_SYMBOL = range(7)
SR_TABLE_BYTES = 25 * 128 * 128 + 5 * 128


@dataclass
class SrResult:
    ret: np.ndarray        # int32 per layout: what consensus() returns
    status: np.ndarray     # uint32 per layout: SR_*
    out_off: np.ndarray    # uint64, n_layouts + 1
    cons_seq: np.ndarray   # uint8, packed
    cons_qual: np.ndarray  # uint8, packed
    n_columns: int
    n_host_columns: int    # device call: columns the host threads finished from the device's sums
    ms_device: float
    ms_host_finish: float

    def seq(self, i):
        a, b = int(self.out_off[i]), int(self.out_off[i + 1])
        return self.cons_seq[a:b].tobytes(), self.cons_qual[a:b].tobytes()


def make_settings(min_qual=0.99, min_clique_size=2, error_correction=False, subreads_needed=False, n_threads=1):
    return N.hc_sr_settings(float(min_qual), int(min_clique_size), int(bool(error_correction)), int(bool(subreads_needed)), int(n_threads))


def _ptr(a):
    return a.ctypes.data if a.size else None


def run(call, layouts, members, settings):
    """call(layouts_ptr, n_layouts, members_ptr, n_members, settings_ref, ret, status, out_off, seq, qual, cap, n_bytes_ref, stats_ref) -> status"""
    layouts = np.ascontiguousarray(layouts, dtype=SR_LAYOUT_DTYPE)
    members = np.ascontiguousarray(members, dtype=SR_MEMBER_DTYPE)
    n = layouts.size
    ret = np.zeros(n, np.int32)
    status = np.zeros(n, np.uint32)
    out_off = np.zeros(n + 1, np.uint64)
    cap = int(np.maximum(layouts["total_len"], 0).astype(np.int64).sum())
    seq = np.zeros(cap, np.uint8)
    qual = np.zeros(cap, np.uint8)
    n_bytes = C.c_uint64(0)
    stats = N.hc_sr_stats()
    N.check(call(_ptr(layouts), n, _ptr(members), members.size, C.byref(settings), ret.ctypes.data if n else None,
                 status.ctypes.data if n else None, out_off.ctypes.data, _ptr(seq), _ptr(qual), cap, C.byref(n_bytes), C.byref(stats)),
            "sr_consensus")
    nb = int(n_bytes.value)
    return SrResult(ret, status, out_off, seq[:nb], qual[:nb], int(stats.n_columns), int(stats.n_host_columns), float(stats.ms_device),
                    float(stats.ms_host_finish))


def edge_layouts(edges, reads):
    """Layouts of edge merges between single-end reads, as sort_vertices type 's' builds them (src/SRBuilder.cpp:33-285).
    edges: hc_edge_rec records (records.EDGE_DTYPE); returns (layouts, members).  A paired read is refused (HcError)."""
    from .host import EDGE_DTYPE

    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    first = reads.read_first_seq.astype(np.int64)
    paired = np.ascontiguousarray((first[1:] - first[:-1]) == 2, dtype=np.uint8)
    lens = np.ascontiguousarray((reads.seq_off[1:] - reads.seq_off[:-1])[first[:-1]], dtype=np.uint32)
    layouts = np.zeros(edges.size, SR_LAYOUT_DTYPE)
    members = np.zeros(2 * edges.size, SR_MEMBER_DTYPE)
    bad = C.c_uint64(0)
    N.check(N.lib.hc_host_sr_edge_layouts(_ptr(edges), edges.size, _ptr(lens), _ptr(paired), reads.n_reads, _ptr(layouts), _ptr(members),
                                          C.byref(bad)), "sr edge_layouts")
    return layouts, members


# ---- edge merges on a graph (hc_graph_merge_pairs, hc_sr_edge_merge) ------------------------------------------------------
SR_SUBREAD_DTYPE = np.dtype([("index1", "<i4"), ("startpos1", "<i4"), ("index2", "<i4"), ("startpos2", "<i4")], align=False)  # hc_sr_subread_info
assert SR_SUBREAD_DTYPE.itemsize == 16
SR_EDGE_OK, SR_EDGE_NO_EDGE, SR_EDGE_BAD_VERTEX, SR_EDGE_READ_MISMATCH, SR_EDGE_PAIRED_NEG_POS, SR_EDGE_BAD_GEOMETRY = range(6)


@dataclass
class SrEdgeLayouts:
    pair_status: np.ndarray   # uint32 per pair: SR_EDGE_*
    first_layout: np.ndarray  # uint64, n_pairs + 1
    layouts: np.ndarray       # SR_LAYOUT_DTYPE, packed in pair order ('l' before 'r')
    members: np.ndarray       # SR_MEMBER_DTYPE, packed
    subreads: np.ndarray      # SR_SUBREAD_DTYPE, (n_pairs, 2): the smaller, the larger vertex (None: the mirror without ret)
    result: SrResult = None   # the device call: hc_sr_consensus' outputs for the layouts


def merge_pairs(call, n_vertices):
    """call(pairs_ptr, cap, n_pairs_ref) -> status; the pairs of getEdgesForMerging (src/GraphAlgos.cpp:112-148) as an (n, 2) uint32 array."""
    pairs = np.zeros((n_vertices // 2 + 1, 2), np.uint32)
    n = C.c_uint64(0)
    N.check(call(pairs.ctypes.data, pairs.shape[0], C.byref(n)), "merge_pairs")
    return pairs[:int(n.value)].copy()


def _edge_buffers(pairs):
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n = pairs.shape[0]
    return pairs, n, np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(2 * n, SR_LAYOUT_DTYPE), np.zeros(6 * n, SR_MEMBER_DTYPE)


def _trim(status, first, layouts, members, subreads, result=None):
    nl = int(first[-1])
    nm = int(layouts["n_members"][:nl].astype(np.int64).sum())
    return SrEdgeLayouts(status, first, layouts[:nl], members[:nm], subreads, result)


def edge_merge(ctx, pairs, vertex_read, vertex_fwd, settings, cap=None):
    """hc_sr_edge_merge on the context's graph and store: constructSuperread's ordering, sort_vertices, consensus and calcSubreadInfo
    (src/SRBuilder.cpp:654-698, 33-285, 413-535, 536-595) for every pair of vertices.  Returns an SrEdgeLayouts with .result set.
    cap: room for the consensus bytes; None asks with cap = 0 first and calls again with exactly the bytes needed."""
    pairs, n, status, first, layouts, members = _edge_buffers(pairs)
    vr = np.ascontiguousarray(vertex_read, dtype=np.uint32)
    vf = np.ascontiguousarray(vertex_fwd, dtype=np.uint8)
    if vr.size != vf.size:
        raise ValueError("vertex_read and vertex_fwd differ in length")
    sub = np.zeros((n, 2), SR_SUBREAD_DTYPE)
    ret, lstat, out_off = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.uint32), np.zeros(2 * n + 1, np.uint64)
    n_bytes = C.c_uint64(0)
    stats = N.hc_sr_stats()

    def once(seq, qual, room):
        return N.lib.hc_sr_edge_merge(ctx, _ptr(pairs), n, _ptr(vr), _ptr(vf), vr.size, C.byref(settings), _ptr(status), first.ctypes.data,
                                      _ptr(layouts), _ptr(members), _ptr(sub), _ptr(ret), _ptr(lstat), out_off.ctypes.data, _ptr(seq), _ptr(qual), room,
                                      C.byref(n_bytes), C.byref(stats))

    if cap is None:
        empty = np.zeros(0, np.uint8)
        rc = once(empty, empty, 0)
        if rc != 0 and n_bytes.value == 0:
            N.check(rc, "sr_edge_merge")
        cap = int(n_bytes.value)
        seq, qual = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        if cap:
            N.check(once(seq, qual, cap), "sr_edge_merge")
    else:
        seq, qual = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        N.check(once(seq, qual, cap), "sr_edge_merge")
    nl, nb = int(first[-1]), int(n_bytes.value)
    res = SrResult(ret[:nl], lstat[:nl], out_off[:nl + 1], seq[:nb], qual[:nb], int(stats.n_columns), int(stats.n_host_columns), float(stats.ms_device),
                   float(stats.ms_host_finish))
    return _trim(status, first, layouts, members, sub, res)


def host_edge_merge_layouts(edges, out_off, reads, pairs, vertex_read, vertex_fwd, settings, ret=None):
    """hc_host_sr_edge_merge_layouts: the layouts (and, given the layouts' ret, the subread infos) of edge_merge on a host graph
    (hc_graph_fetch's edges / out_off) and a ReadSet."""
    from .host import EDGE_DTYPE

    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    oo = np.ascontiguousarray(out_off, dtype=np.uint64)
    pairs, n, status, first, layouts, members = _edge_buffers(pairs)
    vr = np.ascontiguousarray(vertex_read, dtype=np.uint32)
    vf = np.ascontiguousarray(vertex_fwd, dtype=np.uint8)
    sub = None
    if ret is not None:
        ret = np.ascontiguousarray(ret, dtype=np.int32)
        sub = np.zeros((n, 2), SR_SUBREAD_DTYPE)
    N.check(N.lib.hc_host_sr_edge_merge_layouts(_ptr(edges), oo.ctypes.data, oo.size - 1, reads.seq_off.ctypes.data, reads.read_first_seq.ctypes.data,
                                                reads.n_reads, _ptr(pairs), n, _ptr(vr), _ptr(vf), C.byref(settings), _ptr(status), first.ctypes.data,
                                                _ptr(layouts), _ptr(members), None if ret is None else ret.ctypes.data,
                                                None if sub is None else _ptr(sub)), "sr_edge_merge_layouts")
    return _trim(status, first, layouts, members, sub)


# ---- cliques of any size (hc_sr_clique_merge) ------------------------------------------------------------------------------
SR_CLIQUE_TOO_SMALL, SR_CLIQUE_REPEATED_VERTEX = 6, 7
SR_FILTER_NONE, SR_FILTER_GROUPS, SR_FILTER_STABLE, SR_FILTER_HOST = range(4)


@dataclass
class SrCliqueLayouts:
    clique_status: np.ndarray  # uint32 per clique: SR_EDGE_* / SR_CLIQUE_*
    first_layout: np.ndarray   # uint64, n_cliques + 1
    layouts: np.ndarray        # SR_LAYOUT_DTYPE: the FULL lists, packed in clique order ('l' before 'r')
    members: np.ndarray        # SR_MEMBER_DTYPE, packed
    member_vertex: np.ndarray  # uint32 per member: sorted_vertices1 / sorted_vertices2
    member_used: np.ndarray    # uint8 per member: handed to consensus
    layout_filter: np.ndarray  # uint8 per layout: SR_FILTER_*
    subreads: np.ndarray       # SR_SUBREAD_DTYPE per clique vertex, ascending vertex, at clique_off (None: the mirror without ret)
    n_filtered_layouts: int = 0
    n_host_filters: int = 0
    ms_layout: float = 0.0
    ms_host_filter: float = 0.0
    result: SrResult = None    # the device call: hc_sr_consensus' outputs for the USED members

    def used_layouts(self):
        """(layouts, members) of the USED members, as hc_sr_consensus takes them."""
        used = self.member_used.astype(bool)
        before = np.concatenate([[0], np.cumsum(used)]).astype(np.uint64)
        lay = self.layouts.copy()
        fm = self.layouts["first_member"].astype(np.int64)
        lay["first_member"] = before[fm]
        lay["n_members"] = before[fm + self.layouts["n_members"].astype(np.int64)] - before[fm]
        return lay, self.members[used]


def clique_csr(cliques):
    """[[vertex, ...], ...] -> (clique_off uint64, clique_nodes uint32)."""
    off = np.zeros(len(cliques) + 1, np.uint64)
    off[1:] = np.cumsum([len(q) for q in cliques])
    nodes = np.asarray([v for q in cliques for v in q], np.uint32)
    return off, nodes


def _clique_buffers(clique_off, clique_nodes):
    off = np.ascontiguousarray(clique_off, dtype=np.uint64)
    nodes = np.ascontiguousarray(clique_nodes, dtype=np.uint32)
    n, total = off.size - 1, int(off[-1])
    if nodes.size != total:
        raise ValueError("clique_nodes does not hold clique_off[-1] entries")
    return (off, nodes, n, total, np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(2 * n, SR_LAYOUT_DTYPE),
            np.zeros(2 * total, SR_MEMBER_DTYPE), np.zeros(2 * total, np.uint32), np.zeros(2 * total, np.uint8), np.zeros(2 * n, np.uint8))


def _trim_clique(status, first, layouts, members, vertex, used, filt, subreads, stats, result=None):
    nl = int(first[-1])
    nm = int(layouts["n_members"][:nl].astype(np.int64).sum())
    return SrCliqueLayouts(status, first, layouts[:nl], members[:nm], vertex[:nm], used[:nm], filt[:nl], subreads, int(stats.n_filtered_layouts),
                           int(stats.n_host_filters), float(stats.ms_layout), float(stats.ms_host_filter), result)


def clique_merge(ctx, clique_off, clique_nodes, vertex_read, vertex_fwd, settings, cap=None):
    """hc_sr_clique_merge on the context's graph and store: constructSuperread (src/SRBuilder.cpp:654-748) for cliques of any size given as
    a CSR of vertex ids.  Returns an SrCliqueLayouts with .result set.  cap: as edge_merge's."""
    off, nodes, n, total, status, first, layouts, members, vertex, used, filt = _clique_buffers(clique_off, clique_nodes)
    vr = np.ascontiguousarray(vertex_read, dtype=np.uint32)
    vf = np.ascontiguousarray(vertex_fwd, dtype=np.uint8)
    if vr.size != vf.size:
        raise ValueError("vertex_read and vertex_fwd differ in length")
    sub = np.zeros(total, SR_SUBREAD_DTYPE)
    ret, lstat, out_off = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.uint32), np.zeros(2 * n + 1, np.uint64)
    n_bytes = C.c_uint64(0)
    stats = N.hc_sr_clique_stats()

    def once(seq, qual, room):
        return N.lib.hc_sr_clique_merge(ctx, off.ctypes.data, _ptr(nodes), n, _ptr(vr), _ptr(vf), vr.size, C.byref(settings), _ptr(status),
                                        first.ctypes.data, _ptr(layouts), _ptr(members), _ptr(vertex), _ptr(used), _ptr(filt), _ptr(sub), _ptr(ret),
                                        _ptr(lstat), out_off.ctypes.data, _ptr(seq), _ptr(qual), room, C.byref(n_bytes), C.byref(stats))

    if cap is None:
        empty = np.zeros(0, np.uint8)
        rc = once(empty, empty, 0)
        if rc != 0 and n_bytes.value == 0:
            N.check(rc, "sr_clique_merge")
        cap = int(n_bytes.value)
        seq, qual = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        if cap:
            N.check(once(seq, qual, cap), "sr_clique_merge")
    else:
        seq, qual = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        N.check(once(seq, qual, cap), "sr_clique_merge")
    nl, nb = int(first[-1]), int(n_bytes.value)
    res = SrResult(ret[:nl], lstat[:nl], out_off[:nl + 1], seq[:nb], qual[:nb], int(stats.sr.n_columns), int(stats.sr.n_host_columns),
                   float(stats.sr.ms_device), float(stats.sr.ms_host_finish))
    return _trim_clique(status, first, layouts, members, vertex, used, filt, sub, stats, res)


def host_clique_merge_layouts(edges, out_off, reads, clique_off, clique_nodes, vertex_read, vertex_fwd, settings, ret=None):
    """hc_host_sr_clique_merge_layouts: the layouts, filter_subreads' choice and (given the layouts' ret) the subread infos of clique_merge on a
    host graph (hc_graph_fetch's edges / out_off) and a ReadSet."""
    from .host import EDGE_DTYPE

    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    oo = np.ascontiguousarray(out_off, dtype=np.uint64)
    off, nodes, n, total, status, first, layouts, members, vertex, used, filt = _clique_buffers(clique_off, clique_nodes)
    vr = np.ascontiguousarray(vertex_read, dtype=np.uint32)
    vf = np.ascontiguousarray(vertex_fwd, dtype=np.uint8)
    sub = None
    if ret is not None:
        ret = np.ascontiguousarray(ret, dtype=np.int32)
        sub = np.zeros(total, SR_SUBREAD_DTYPE)
    stats = N.hc_sr_clique_stats()
    N.check(N.lib.hc_host_sr_clique_merge_layouts(_ptr(edges), oo.ctypes.data, oo.size - 1, reads.seq_off.ctypes.data, reads.read_first_seq.ctypes.data,
                                                  reads.n_reads, off.ctypes.data, _ptr(nodes), n, _ptr(vr), _ptr(vf), C.byref(settings), _ptr(status),
                                                  first.ctypes.data, _ptr(layouts), _ptr(members), _ptr(vertex), _ptr(used), _ptr(filt),
                                                  None if ret is None else ret.ctypes.data, None if sub is None else _ptr(sub), C.byref(stats)),
            "sr_clique_merge_layouts")
    return _trim_clique(status, first, layouts, members, vertex, used, filt, sub, stats)


def host_clique_filter(vertex, endpos, num, base_vertex, tie_order=0):
    """hc_host_sr_clique_filter: filter_subreads' selection (src/SRBuilder.cpp:597-622) for one layout -> (used uint8 per entry, SR_FILTER_*)."""
    vertex = np.ascontiguousarray(vertex, dtype=np.uint32)
    endpos = np.ascontiguousarray(endpos, dtype=np.int32)
    used = np.zeros(vertex.size, np.uint8)
    cls = C.c_uint32(0)
    N.check(N.lib.hc_host_sr_clique_filter(_ptr(vertex), _ptr(endpos), vertex.size, int(num), int(base_vertex), int(tie_order), _ptr(used),
                                           C.byref(cls)), "sr_clique_filter")
    return used, int(cls.value)


def column(nucleotides, qualities, min_qual=0.99):
    """consensus_pos for one column given as byte strings: (nucleotide, quality byte), or None where it returns 0."""
    out = (C.c_uint8 * 2)()
    ok = N.lib.hc_host_sr_column(bytes(nucleotides), bytes(qualities), len(nucleotides), float(min_qual), out)
    return (out[0], out[1]) if ok else None


def table(min_qual, n_q):
    t = np.zeros(SR_TABLE_BYTES, np.uint8)
    N.check(N.lib.hc_host_sr_table(float(min_qual), int(n_q), t.ctypes.data), "hc_host_sr_table")
    return t


# ---- self-overlapping paired super-reads (hc_sr_merge_self_overlaps) ----------------------------------------------------
SR_PAIR_DTYPE = np.dtype([("off1", "<u8"), ("off2", "<u8"), ("len1", "<u4"), ("len2", "<u4")], align=False)  # hc_sr_pair
assert SR_PAIR_DTYPE.itemsize == 24
SR_SELF_NONE, SR_SELF_MERGED, SR_SELF_BAD_PAIR, SR_SELF_BAD_SYMBOL = range(4)


@dataclass
class SrSelfResult:
    overlap_pos: np.ndarray  # int32 per pair: the offset taken, or -1
    score: np.ndarray        # float64 per pair: overlap_score at that offset, or 0
    status: np.ndarray       # uint32 per pair: SR_SELF_*
    out_off: np.ndarray      # uint64, n_pairs + 1
    merged_seq: np.ndarray   # uint8, packed
    merged_qual: np.ndarray  # uint8, packed
    n_merged: int
    n_host_pairs: int        # device call: pairs the host threads decided
    n_offsets: int
    ms_device: float
    ms_host: float

    def merged(self, i):
        a, b = int(self.out_off[i]), int(self.out_off[i + 1])
        return self.merged_seq[a:b].tobytes(), self.merged_qual[a:b].tobytes()


def make_self_settings(min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=1):
    return N.hc_sr_self_settings(float(min_score), float(min_qual), int(min_overlap), int(n_threads))


def pack_pairs(mates):
    """[(seq1, qual1, seq2, qual2) as bytes] -> (seq, qual, pairs): the packed buffers hc_sr_consensus would have written."""
    pairs = np.zeros(len(mates), SR_PAIR_DTYPE)
    s, q, at = [], [], 0
    for i, (s1, q1, s2, q2) in enumerate(mates):
        pairs[i] = (at, at + len(s1), len(s1), len(s2))
        s += [s1, s2]
        q += [q1, q2]
        at += len(s1) + len(s2)
    return np.frombuffer(b"".join(s), np.uint8), np.frombuffer(b"".join(q), np.uint8), pairs


def run_self(call, seq, qual, pairs, settings, count_first=True):
    """call(seq, qual, n_bytes, pairs, n_pairs, settings_ref, pos, score, status, out_off, mseq, mqual, cap, n_out_ref, stats_ref) -> status.
    count_first: ask with cap = 0, then fetch; otherwise one call with room for every pair merged at its first offset."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    pairs = np.ascontiguousarray(pairs, dtype=SR_PAIR_DTYPE)
    if seq.size != qual.size:
        raise ValueError("seq and qual differ in length")
    n = pairs.size
    pos = np.zeros(n, np.int32)
    score = np.zeros(n, np.float64)
    status = np.zeros(n, np.uint32)
    out_off = np.zeros(n + 1, np.uint64)
    n_out = C.c_uint64(0)
    stats = N.hc_sr_self_stats()

    def once(mseq, mqual, cap):
        return call(_ptr(seq), _ptr(qual), seq.size, _ptr(pairs), n, C.byref(settings), _ptr(pos), _ptr(score), _ptr(status), out_off.ctypes.data,
                    _ptr(mseq), _ptr(mqual), cap, C.byref(n_out), C.byref(stats))

    empty = np.zeros(0, np.uint8)
    if count_first:
        rc = once(empty, empty, 0)
        if rc != 0 and n_out.value == 0:
            N.check(rc, "sr_merge_self_overlaps")
        cap = int(n_out.value)
    else:
        cap = int(pairs["len1"].astype(np.int64).sum() + pairs["len2"].astype(np.int64).sum())
    mseq = np.zeros(cap, np.uint8)
    mqual = np.zeros(cap, np.uint8)
    if cap or not count_first:
        N.check(once(mseq, mqual, cap), "sr_merge_self_overlaps")
    nb = int(n_out.value)
    return SrSelfResult(pos, score, status, out_off, mseq[:nb], mqual[:nb], int(stats.n_merged), int(stats.n_host_pairs), int(stats.n_offsets),
                        float(stats.ms_device), float(stats.ms_host))


# ---- the same from the kept consensus bytes (hc_sr_merge_self_overlaps_kept, hc_sr_kept_load, hc_sr_kept_fetch) -------------
def kept_load(ctx, seq, qual):
    """hc_sr_kept_load: the caller's packed bytes become the kept consensus bytes of the context."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    if seq.size != qual.size:
        raise ValueError("seq and qual differ in length")
    N.check(N.lib.hc_sr_kept_load(ctx, _ptr(seq), _ptr(qual), seq.size), "sr_kept_load")


def kept_size(ctx):
    n = C.c_uint64(0)
    N.check(N.lib.hc_sr_kept_fetch(ctx, 0, 0, None, None, C.byref(n)), "sr_kept_fetch")
    return int(n.value)


def kept_fetch(ctx, off=0, n=None):
    """hc_sr_kept_fetch: (seq, qual) = bytes [off, off + n) of the kept consensus bytes; n = None: from off to the end."""
    if n is None:
        n = kept_size(ctx) - int(off)
    seq, qual = np.zeros(max(int(n), 0), np.uint8), np.zeros(max(int(n), 0), np.uint8)
    kept = C.c_uint64(0)
    N.check(N.lib.hc_sr_kept_fetch(ctx, int(off), int(n), _ptr(seq), _ptr(qual), C.byref(kept)), "sr_kept_fetch")
    return seq, qual


@dataclass
class SrSelfKeptResult(SrSelfResult):
    """out_off holds ABSOLUTE offsets into the kept bytes (out_off[0] = the kept size before the call); merged_seq / merged_qual are
    empty: the merged reads stay on the device.  merged(i) and relative() read them back with hc_sr_kept_fetch."""
    ctx: object = None

    def merged(self, i):
        a, b = int(self.out_off[i]), int(self.out_off[i + 1])
        s, q = kept_fetch(self.ctx, a, b - a)
        return s.tobytes(), q.tobytes()

    def relative(self):
        """The result in the host-input call's form: offsets from 0 and the appended bytes on the host, in one fetch."""
        base = int(self.out_off[0])
        s, q = kept_fetch(self.ctx, base, int(self.out_off[-1]) - base)
        return SrSelfResult(self.overlap_pos, self.score, self.status, self.out_off - np.uint64(base), s, q, self.n_merged, self.n_host_pairs,
                            self.n_offsets, self.ms_device, self.ms_host)


def run_self_kept(ctx, pairs, settings):
    """hc_sr_merge_self_overlaps_kept on the context's kept consensus bytes.  Returns an SrSelfKeptResult."""
    pairs = np.ascontiguousarray(pairs, dtype=SR_PAIR_DTYPE)
    n = pairs.size
    pos = np.zeros(n, np.int32)
    score = np.zeros(n, np.float64)
    status = np.zeros(n, np.uint32)
    out_off = np.zeros(n + 1, np.uint64)
    n_out = C.c_uint64(0)
    stats = N.hc_sr_self_stats()
    N.check(N.lib.hc_sr_merge_self_overlaps_kept(ctx, _ptr(pairs), n, C.byref(settings), _ptr(pos), _ptr(score), _ptr(status), out_off.ctypes.data,
                                                 C.byref(n_out), C.byref(stats)), "sr_merge_self_overlaps_kept")
    assert int(out_off[-1] - out_off[0]) == int(n_out.value)
    empty = np.zeros(0, np.uint8)
    return SrSelfKeptResult(pos, score, status, out_off, empty, empty, int(stats.n_merged), int(stats.n_host_pairs), int(stats.n_offsets),
                            float(stats.ms_device), float(stats.ms_host), ctx)
