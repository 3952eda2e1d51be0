"""Python face of include/hcedge_host.h: the host-side stage (FastqStorage / OverlapGraph /
EdgeCalculator mirrors in csrc/host/) and its GPU-free pieces."""
import ctypes as C

import numpy as np

from . import _native as N
from .records import OVERLAP_DTYPE, Settings

_vp = C.c_void_p

EDGE_DTYPE = np.dtype(
    [("score", "<f8"), ("mismatch_rate", "<f8"), ("pos1", "<i4"), ("pos2", "<i4"), ("pos3", "<i4"), ("pos4", "<i4"),
     ("ori1", "u1"), ("ori2", "u1"), ("ord", "u1"), ("pad", "u1"), ("read1", "<u4"), ("read2", "<u4"), ("_p2", "<u4"),
     ("v1", "<u8"), ("v2", "<u8"), ("perc", "<i4"), ("len0", "<i4"), ("len1", "<i4"), ("len2", "<i4")], align=False)
assert EDGE_DTYPE.itemsize == 80
# hc_read_geom (include/hcedge.h): what Edge::ext_len reads of a read, by read index
READ_GEOM_DTYPE = np.dtype([("len1", "<u4"), ("len2", "<u4"), ("paired", "u1"), ("pad", "u1", (3,))], align=False)
assert READ_GEOM_DTYPE.itemsize == 12


class hc_ec_paths(C.Structure):
    _fields_ = [("singles_file", C.c_char_p), ("paired1_file", C.c_char_p), ("paired2_file", C.c_char_p),
                ("id_correspondence", C.c_char_p), ("overlaps_file", C.c_char_p), ("output_dir", C.c_char_p),
                ("max_reads", C.c_uint64)]


class hc_ec_counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ("self_overlap_count", "inclusion_count", "dup_count", "edges_added", "nonedges_written",
                 "prefilter_rejected", "malformed_lines", "lines_read", "scored", "ambiguous", "silently_dropped")] + \
               [(k, C.c_double) for k in ("t_parse", "t_score", "t_insert", "t_write")] + \
               [(k, C.c_uint64) for k in ("device_blocks", "host_blocks", "regrown_blocks", "host_lines")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class hc_overlap_fields(C.Structure):
    _fields_ = [("id1", C.c_uint64), ("id2", C.c_uint64), ("pos1", C.c_uint32), ("pos2", C.c_uint32),
                ("perc1", C.c_uint32), ("perc2", C.c_uint32), ("len1", C.c_uint32), ("len2", C.c_uint32),
                ("perc", C.c_uint32), ("ord", C.c_char), ("ori1", C.c_char), ("ori2", C.c_char), ("type1", C.c_char),
                ("type2", C.c_char), ("pad", C.c_char * 3)]


class hc_fastq_view(C.Structure):
    _fields_ = [("bases", _vp), ("quals", _vp), ("seq_off", _vp), ("read_first_seq", _vp), ("read_ids", _vp),
                ("n_reads", C.c_uint32), ("n_seq", C.c_uint32), ("n_single", C.c_uint32), ("n_paired", C.c_uint32)]


_sig = {
    "hc_ec_open": (C.c_int, [C.POINTER(_vp), C.POINTER(N.hc_settings), C.POINTER(hc_ec_paths)]),
    "hc_ec_construct_edges": (C.c_int, [_vp]),
    "hc_ec_construct_edges_sorted": (C.c_int, [_vp]),
    "hc_ec_construct_edges_from_reads": (C.c_int, [_vp, C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hc_ec_construct_edges_from_sfo": (C.c_int, [_vp, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "hc_ec_construct_edges_from_store": (C.c_int, [_vp, C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_int)]),
    "hc_ec_device_count": (C.c_uint32, [_vp]),
    "hc_ec_get_counters": (C.c_int, [_vp, C.POINTER(hc_ec_counters)]),
    "hc_ec_read_count": (C.c_uint64, [_vp]),
    "hc_ec_vertex_count": (C.c_uint64, [_vp]),
    "hc_ec_edge_count": (C.c_uint64, [_vp]),
    "hc_ec_get_edges": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_ec_get_inclusions": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_ec_overlap_score": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hc_ec_close": (C.c_int, [_vp]),
    "hc_ec_keep_devices": (C.c_int, [C.c_int]),
    "hc_ec_fastq_on_device": (C.c_int, [C.c_int]),
    "hc_ec_fastq_was_on_device": (C.c_int, [_vp]),
    "hc_ec_get_read_seq": (C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_host_split_line": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int, _vp, _vp, C.c_int]),
    "hc_host_parse_overlap": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(hc_overlap_fields), C.c_char_p]),
    "hc_host_fastq_load": (C.c_int, [C.POINTER(_vp), C.POINTER(hc_ec_paths), C.POINTER(hc_fastq_view)]),
    "hc_host_fastq_free": (C.c_int, [_vp]),
    "hc_host_parse_file": (C.c_int, [C.POINTER(N.hc_settings), _vp, C.c_char_p, _vp, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(hc_ec_counters)]),
    "hc_host_parse_text": (C.c_int, [C.POINTER(N.hc_settings), _vp, C.c_char_p, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(hc_ec_counters)]),
    "hc_sfo2overlaps": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_sfo_records_to_overlaps": (C.c_int, [_vp, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_host_write_sfo": (C.c_int, [C.c_char_p, _vp, C.c_uint64]),
    "hc_ec_sam_on_device": (C.c_int, [C.c_int]),
    "hc_host_sam_read": (C.c_int, [C.POINTER(_vp), C.c_char_p, C.c_char_p, C.c_char_p, _vp]),
    "hc_host_sam_free": (C.c_int, [_vp]),
    "hc_host_sam_records_to_lines": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_host_sam_write_lines": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_char_p]),
    "hc_host_sam2overlaps": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64)]),
    "hc_ec_construct_edges_from_sam": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "hc_host_write_overlaps": (C.c_int, [C.c_char_p, _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.c_uint32]),
    "hc_host_graph_new": (C.c_int, [C.POINTER(_vp), C.c_uint64, C.POINTER(N.hc_settings)]),
    "hc_host_graph_insert": (C.c_int, [_vp, _vp]),
    "hc_host_graph_resolve": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_host_graph_adopt": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "hc_host_graph_add_equivalent_edges": (C.c_int, [_vp]),
    "hc_host_graph_sort_edges": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_host_graph_get_in_lists": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "hc_ec_sort_edges": (C.c_int, [_vp]),
    "hc_ec_get_in_lists": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "hc_host_graph_get": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp, C.POINTER(hc_ec_counters)]),
    "hc_host_graph_free": (C.c_int, [_vp]),
    "hc_host_graph_remove_inclusions": (C.c_int, [_vp]),
    "hc_host_graph_remove_transitive_edges": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(N.hc_clean_counts)]),
    "hc_host_graph_get_inclusion_edges": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hc_host_graph_remove_tips": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(N.hc_tip_counts)]),
    "hc_host_graph_remove_branches": (C.c_int, [_vp, C.POINTER(N.hc_branch_counts)]),
    "hc_host_graph_label_vertices": (C.c_int, [_vp, C.POINTER(N.hc_label_settings), C.POINTER(N.hc_label_counts)]),
    "hc_host_graph_get_orientations": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_host_label_rand": (C.c_int, [C.c_uint32, _vp, C.c_uint64]),
    "hc_host_label_shuffle": (C.c_int, [C.c_uint32, _vp, C.c_uint64]),
    "hc_host_graph_get_branching_edges": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_host_graph_get_tip_reads": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_host_graph_write_text": (C.c_int, [_vp, C.c_uint32, C.POINTER(N.hc_graph_text_settings), _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64,
                                           C.POINTER(N.hc_graph_text_counts)]),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(N.lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def _b(s):
    return None if s is None else (s if isinstance(s, bytes) else str(s).encode())


def make_paths(singles=None, paired1=None, paired2=None, ids=None, overlaps=None, output_dir="", max_reads=0):
    return hc_ec_paths(_b(singles), _b(paired1), _b(paired2), _b(ids), _b(overlaps), _b(output_dir), max_reads)


def split_line(line, allow_spaces=False, max_fields=32):
    raw = line if isinstance(line, bytes) else line.encode()
    off = np.zeros(max_fields, np.uint32)
    ln = np.zeros(max_fields, np.uint32)
    n = N.lib.hc_host_split_line(raw, len(raw), 1 if allow_spaces else 0, off.ctypes.data, ln.ctypes.data, max_fields)
    return n, [raw[int(off[i]):int(off[i] + ln[i])].decode() for i in range(min(n, max_fields))]


def parse_overlap(line, allow_spaces=False, general_only=False):
    raw = line if isinstance(line, bytes) else line.encode()
    o = hc_overlap_fields()
    text = C.create_string_buffer(256)
    rc = N.lib.hc_host_parse_overlap(raw, len(raw), (1 if allow_spaces else 0) | (2 if general_only else 0), C.byref(o), text)
    if rc:
        return rc, None
    return 0, {"id1": o.id1, "id2": o.id2, "pos1": o.pos1, "pos2": o.pos2, "ord": o.ord.decode(), "ori1": o.ori1.decode(),
               "ori2": o.ori2.decode(), "type1": o.type1.decode(), "type2": o.type2.decode(), "perc": o.perc,
               "len1": o.len1, "len2": o.len2, "line": text.value.decode()}


def write_overlaps(path, recs, reads, n_threads=0):
    """Candidate records -> 13-column overlaps file (hc_host_write_overlaps): what synth.records_to_lines does, natively."""
    recs = np.ascontiguousarray(recs)
    ids = np.ascontiguousarray(reads.read_ids, dtype=np.uint64)
    rfs = np.asarray(reads.read_first_seq)
    paired = np.ascontiguousarray((rfs[1:] - rfs[:-1]) == 2, dtype=np.uint8)
    N.check(N.lib.hc_host_write_overlaps(_b(path), recs.ctypes.data, recs.size, ids.ctypes.data, paired.ctypes.data, ids.size, n_threads),
            "hc_host_write_overlaps")


def write_sfo(path, recs):
    """SFO records (records.SFO_DTYPE) as the text file rust-overlaps writes."""
    recs = np.ascontiguousarray(recs)
    N.check(N.lib.hc_host_write_sfo(_b(path), recs.ctypes.data, recs.size), "hc_host_write_sfo")


def sfo_records_to_overlaps(recs, out_path, num_singles, num_pairs):
    """SFO records straight to the 13-column overlaps file (hc_sfo_records_to_overlaps): write_sfo + sfo2overlaps
    without the intermediate text."""
    recs = np.ascontiguousarray(recs)
    n = C.c_uint64()
    N.check(N.lib.hc_sfo_records_to_overlaps(recs.ctypes.data, recs.size, _b(out_path), num_singles, num_pairs, C.byref(n)),
            "hc_sfo_records_to_overlaps")
    return int(n.value)


def sfo2overlaps(sfo_path, out_path, num_singles, num_pairs):
    """scripts/sfo2overlaps.py --in --out --num_singles --num_pairs, natively (hc_sfo2overlaps)."""
    n = C.c_uint64()
    N.check(N.lib.hc_sfo2overlaps(_b(sfo_path), _b(out_path), num_singles, num_pairs, C.byref(n)), "hc_sfo2overlaps")
    return int(n.value)


class hc_sam_view(C.Structure):
    _fields_ = [("alns", _vp), ("recs", _vp), ("ops", _vp), ("id_text", _vp), ("ref_len", _vp)] + \
               [(k, C.c_uint64) for k in ("n_alns", "n_recs", "n_singles", "n_ops", "n_id_bytes", "n_refs")]


class SamRecords:
    """SAM records (include/hcedge.h: hc_sam_aln, hc_sam_rec, hc_sam_op) with the reference lengths and the ids' text: what
    hc_host_sam_read makes of the files (SamRecords.read), or arrays a caller built."""

    def __init__(self, alns, recs, ops, ref_len, id_text=b""):
        from .records import SAM_ALN_DTYPE, SAM_OP_DTYPE, SAM_REC_DTYPE

        self.alns = np.ascontiguousarray(alns, dtype=SAM_ALN_DTYPE)
        self.recs = np.ascontiguousarray(recs, dtype=SAM_REC_DTYPE)
        self.ops = np.ascontiguousarray(ops, dtype=SAM_OP_DTYPE)
        self.ref_len = np.ascontiguousarray(ref_len, dtype=np.uint64)
        self.id_text = bytes(id_text)

    @classmethod
    def read(cls, sam_s, sam_p, ref_fasta):
        """scripts/sam2overlaps.py's reading of the two SAM files (None: absent) and the FASTA (hc_host_sam_read)."""
        from .records import SAM_ALN_DTYPE, SAM_OP_DTYPE, SAM_REC_DTYPE

        h, v = _vp(), hc_sam_view()
        N.check(N.lib.hc_host_sam_read(C.byref(h), _b(sam_s), _b(sam_p), _b(ref_fasta), C.byref(v)), "hc_host_sam_read")
        try:
            def arr(ptr, n, dt):
                return np.frombuffer(C.string_at(ptr, n * dt.itemsize), dtype=dt).copy() if n else np.zeros(0, dt)

            return cls(arr(v.alns, v.n_alns, SAM_ALN_DTYPE), arr(v.recs, v.n_recs, SAM_REC_DTYPE), arr(v.ops, v.n_ops, SAM_OP_DTYPE),
                       arr(v.ref_len, v.n_refs, np.dtype("<u8")), C.string_at(v.id_text, v.n_id_bytes) if v.n_id_bytes else b"")
        finally:
            N.lib.hc_host_sam_free(h)

    @property
    def n_singles(self):
        from .records import SAM_NONE

        return int((self.recs["second"] == SAM_NONE).sum())

    def ids(self):
        """the alignments' ids as bytes"""
        return [self.id_text[int(a["id_off"]):int(a["id_off"]) + int(a["id_len"])] for a in self.alns]

    def _view(self):
        self._idbuf = C.create_string_buffer(self.id_text, len(self.id_text) + 1)
        return hc_sam_view(self.alns.ctypes.data, self.recs.ctypes.data, self.ops.ctypes.data, C.addressof(self._idbuf), self.ref_len.ctypes.data,
                           self.alns.size, self.recs.size, self.n_singles, self.ops.size, len(self.id_text), self.ref_len.size)

    def to_lines(self, min_overlap_len):
        """hc_host_sam_records_to_lines: the script's loops as written -> (lines as records.LINE_DTYPE, src: the two alignments of each line)."""
        from .records import LINE_DTYPE

        v, n = self._view(), C.c_uint64()
        N.check(N.lib.hc_host_sam_records_to_lines(C.byref(v), int(min_overlap_len), None, None, 0, C.byref(n)), "hc_host_sam_records_to_lines")
        lines, src = np.zeros(n.value, LINE_DTYPE), np.zeros((n.value, 2), np.uint32)
        if n.value:
            N.check(N.lib.hc_host_sam_records_to_lines(C.byref(v), int(min_overlap_len), lines.ctypes.data, src.ctypes.data, n.value, C.byref(n)),
                    "hc_host_sam_records_to_lines")
        return lines, src

    def write_lines(self, lines, src, out_path):
        """hc_host_sam_write_lines: lines as the script writes them; src None: the ids as decimal numbers (lines from the device)."""
        lines = np.ascontiguousarray(lines)
        v = self._view()
        s = None if src is None else np.ascontiguousarray(src, dtype=np.uint32)
        N.check(N.lib.hc_host_sam_write_lines(C.byref(v), lines.ctypes.data if lines.size else None, None if s is None else s.ctypes.data, lines.size,
                                              _b(out_path)), "hc_host_sam_write_lines")


def sam2overlaps(sam_s, sam_p, ref_fasta, out_path, min_overlap_len=0):
    """scripts/sam2overlaps.py --sam_s --sam_p --ref --out --min_overlap_len, natively (hc_host_sam2overlaps).  Returns the number of lines."""
    n = C.c_uint64()
    N.check(N.lib.hc_host_sam2overlaps(_b(sam_s), _b(sam_p), _b(ref_fasta), _b(out_path), int(min_overlap_len), C.byref(n)), "hc_host_sam2overlaps")
    return int(n.value)


class Fastq:
    """FastqStorage alone (no device)."""

    def __init__(self, singles=None, paired1=None, paired2=None, ids=None, max_reads=0):
        self._h = _vp()
        self._paths = make_paths(singles, paired1, paired2, ids, max_reads=max_reads)
        v = hc_fastq_view()
        N.check(N.lib.hc_host_fastq_load(C.byref(self._h), C.byref(self._paths), C.byref(v)), "hc_host_fastq_load")
        self.n_reads, self.n_seq, self.n_single, self.n_paired = v.n_reads, v.n_seq, v.n_single, v.n_paired

        def arr(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()

        self.seq_off = arr(v.seq_off, v.n_seq + 1, np.uint64)
        total = int(self.seq_off[-1]) if v.n_seq else 0
        self.bases = arr(v.bases, total, np.uint8)
        self.quals = arr(v.quals, total, np.uint8)
        self.read_first_seq = arr(v.read_first_seq, v.n_reads + 1, np.uint32)
        self.read_ids = arr(v.read_ids, v.n_reads, np.uint64)

    def readset(self):
        from .readstore import ReadSet

        return ReadSet(self.bases, self.quals, self.seq_off, self.read_first_seq, self.read_ids)

    def parse_file(self, settings: Settings, overlaps_path):
        cs = settings.to_c()
        n = C.c_uint64()
        c = hc_ec_counters()
        N.check(N.lib.hc_host_parse_file(C.byref(cs), self._h, _b(overlaps_path), None, 0, C.byref(n), C.byref(c)),
                "hc_host_parse_file")
        out = np.zeros(n.value, dtype=OVERLAP_DTYPE)
        N.check(N.lib.hc_host_parse_file(C.byref(cs), self._h, _b(overlaps_path), out.ctypes.data, n.value, C.byref(n),
                                         C.byref(c)), "hc_host_parse_file")
        return out, c.as_dict()

    def parse_text(self, settings: Settings, text):
        """hc_host_parse_text: the overlaps file's text in memory through the same parser."""
        raw = text if isinstance(text, bytes) else text.encode()
        cs = settings.to_c()
        n = C.c_uint64()
        c = hc_ec_counters()
        N.check(N.lib.hc_host_parse_text(C.byref(cs), self._h, raw, len(raw), None, 0, C.byref(n), C.byref(c)), "hc_host_parse_text")
        out = np.zeros(n.value, dtype=OVERLAP_DTYPE)
        N.check(N.lib.hc_host_parse_text(C.byref(cs), self._h, raw, len(raw), out.ctypes.data, n.value, C.byref(n), C.byref(c)), "hc_host_parse_text")
        return out, c.as_dict()

    def close(self):
        if self._h:
            N.lib.hc_host_fastq_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostGraph:
    """The serial insert of process_overlaps on a bare graph (no device)."""

    def __init__(self, n_vertices, settings: Settings):
        self._h = _vp()
        self.V = n_vertices
        self._cs = settings.to_c()
        N.check(N.lib.hc_host_graph_new(C.byref(self._h), n_vertices, C.byref(self._cs)), "hc_host_graph_new")

    def insert(self, edge_rec):
        e = np.ascontiguousarray(edge_rec, dtype=EDGE_DTYPE).reshape(1)
        return N.lib.hc_host_graph_insert(self._h, e.ctypes.data)

    def resolve(self, edge_recs):
        e = np.ascontiguousarray(edge_recs, dtype=EDGE_DTYPE)
        return N.lib.hc_host_graph_resolve(self._h, e.ctypes.data, e.shape[0])

    def adopt(self, edges, out_off, in_nodes, in_off, inclusions=None):
        """OverlapGraph::adopt_csr: the CSR form hc_graph_fetch returns, into this (empty) graph."""
        e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        oo, io = np.ascontiguousarray(out_off, np.uint64), np.ascontiguousarray(in_off, np.uint64)
        inn = np.ascontiguousarray(in_nodes, np.uint32)
        inc = None if inclusions is None else np.ascontiguousarray(inclusions, np.uint8)
        return N.lib.hc_host_graph_adopt(self._h, e.ctypes.data, oo.ctypes.data, inn.ctypes.data, io.ctypes.data, None if inc is None else inc.ctypes.data)

    def add_equivalent_edges(self):
        return N.lib.hc_host_graph_add_equivalent_edges(self._h)

    def sort_edges(self, len_by_read):
        """OverlapGraph::sortEdges (src/OverlapGraph.cpp:722-764); len_by_read[r] = total length of read r."""
        L = np.ascontiguousarray(len_by_read, dtype=np.uint32)
        N.check(N.lib.hc_host_graph_sort_edges(self._h, L.ctypes.data, L.size), "hc_host_graph_sort_edges")

    def in_lists(self, n_edges):
        off = np.zeros(self.V + 1, np.uint64)
        nodes = np.zeros(max(n_edges, 1), np.uint64)
        N.check(N.lib.hc_host_graph_get_in_lists(self._h, off.ctypes.data, nodes.ctypes.data, n_edges), "hc_host_graph_get_in_lists")
        return off, nodes[:n_edges]

    def remove_inclusions(self):
        """OverlapGraph::removeInclusions (src/GraphAlgos.cpp:20-48); the groups: inclusion_edges()."""
        N.check(N.lib.hc_host_graph_remove_inclusions(self._h), "hc_host_graph_remove_inclusions")

    def remove_transitive_edges(self, remove_trans, branch_reduction=False):
        """OverlapGraph::removeTransitiveEdges (src/GraphAlgos.cpp:938-1077); returns the hc_clean_counts as a dict."""
        c = N.hc_clean_counts()
        N.check(N.lib.hc_host_graph_remove_transitive_edges(self._h, remove_trans, 1 if branch_reduction else 0, C.byref(c)),
                "hc_host_graph_remove_transitive_edges")
        return c.as_dict()

    def inclusion_edges(self):
        """OverlapGraph::inclusion_edges (every removeInclusions call so far): (group offsets, records)."""
        ng, n = C.c_uint64(), C.c_uint64()
        N.check(N.lib.hc_host_graph_get_inclusion_edges(self._h, None, 0, None, 0, C.byref(ng), C.byref(n)), "hc_host_graph_get_inclusion_edges")
        off = np.zeros(ng.value + 1, np.uint64)
        out = np.zeros(n.value, dtype=EDGE_DTYPE)
        N.check(N.lib.hc_host_graph_get_inclusion_edges(self._h, off.ctypes.data, off.size, out.ctypes.data if out.size else None, out.size,
                                                        C.byref(ng), C.byref(n)), "hc_host_graph_get_inclusion_edges")
        return off, out

    def remove_tips(self, max_tip_len, read_geom):
        """OverlapGraph::removeTips (src/GraphAlgos.cpp:543-637); read_geom (READ_GEOM_DTYPE) by read index.  Returns hc_tip_counts as a dict."""
        rg = np.ascontiguousarray(read_geom, dtype=READ_GEOM_DTYPE)
        c = N.hc_tip_counts()
        N.check(N.lib.hc_host_graph_remove_tips(self._h, max_tip_len, rg.ctypes.data if rg.size else None, rg.shape[0], C.byref(c)),
                "hc_host_graph_remove_tips")
        return c.as_dict()

    def remove_branches(self):
        """OverlapGraph::removeBranches (src/GraphAlgos.cpp:835-936); returns hc_branch_counts as a dict."""
        c = N.hc_branch_counts()
        N.check(N.lib.hc_host_graph_remove_branches(self._h, C.byref(c)), "hc_host_graph_remove_branches")
        return c.as_dict()

    def label_vertices(self, resolve_orientations=True, add_duplicates=False, n_reads=0):
        """OverlapGraph::vertexLabellingHeuristic + checkDuplicateEdges (src/GraphAlgos.cpp:150-349, src/OverlapGraph.cpp:578-605) with the
        contract of hc_graph_label_vertices.  Returns (vertex_orientations as bytes, hc_label_counts as a dict)."""
        st, c = N.label_settings(resolve_orientations, add_duplicates, n_reads), N.hc_label_counts()
        N.check(N.lib.hc_host_graph_label_vertices(self._h, C.byref(st), C.byref(c)), "hc_host_graph_label_vertices")
        fwd = np.zeros(self.V, np.uint8)
        N.check(N.lib.hc_host_graph_get_orientations(self._h, fwd.ctypes.data if self.V else None, self.V), "hc_host_graph_get_orientations")
        return fwd, c.as_dict()

    def branching_edges(self):
        """OverlapGraph::branching_edges: what removeTips / removeBranches removed so far, in removal order."""
        n = C.c_uint64()
        N.check(N.lib.hc_host_graph_get_branching_edges(self._h, None, 0, C.byref(n)), "hc_host_graph_get_branching_edges")
        out = np.zeros(n.value, dtype=EDGE_DTYPE)
        if out.size:
            N.check(N.lib.hc_host_graph_get_branching_edges(self._h, out.ctypes.data, out.size, C.byref(n)), "hc_host_graph_get_branching_edges")
        return out

    def tip_reads(self, n_reads):
        """Read::is_tip() of reads [0, n_reads) as bytes."""
        out = np.zeros(n_reads, np.uint8)
        N.check(N.lib.hc_host_graph_get_tip_reads(self._h, out.ctypes.data if n_reads else None, n_reads), "hc_host_graph_get_tip_reads")
        return out

    def write_text(self, kind, edge_threshold=0.0, merge_contigs=0.0, n_singles=0, bases=None, seq_off=None, read_first_seq=None):
        """hc_host_graph_write_text: graph.txt ("cliques"), digraph.txt ("digraph") or a GFA file ("gfa") of this graph as (bytes, counts);
        the reads (GFA only): bases, seq_off (n_seq + 1), read_first_seq (n_reads + 1).  Counts first, then the text."""
        st = N.hc_graph_text_settings(edge_threshold, merge_contigs, n_singles)
        c = N.hc_graph_text_counts()
        k = N.GRAPH_TEXT_KINDS.get(kind, kind)
        b = None if bases is None else np.ascontiguousarray(bases, np.uint8)
        so = None if seq_off is None else np.ascontiguousarray(seq_off, np.uint64)
        fs = None if read_first_seq is None else np.ascontiguousarray(read_first_seq, np.uint32)
        args = (None if b is None or not b.size else b.ctypes.data, None if so is None else so.ctypes.data, None if fs is None else fs.ctypes.data,
                0 if fs is None else fs.size - 1)
        rc = N.lib.hc_host_graph_write_text(self._h, k, C.byref(st), *args, None, 0, C.byref(c))
        if rc == 0 or c.n_bytes == 0:  # an empty text, a failed assert, or a refusal
            N.check(rc, "hc_host_graph_write_text")
            return b"", c.as_dict()
        out = np.empty(int(c.n_bytes), np.uint8)
        N.check(N.lib.hc_host_graph_write_text(self._h, k, C.byref(st), *args, out.ctypes.data, out.size, C.byref(c)), "hc_host_graph_write_text")
        return out.tobytes(), c.as_dict()

    def get(self):
        n = C.c_uint64()
        c = hc_ec_counters()
        inc = np.zeros(self.V, np.uint8)
        N.check(N.lib.hc_host_graph_get(self._h, None, 0, C.byref(n), None, None), "hc_host_graph_get")
        out = np.zeros(n.value, dtype=EDGE_DTYPE)
        N.check(N.lib.hc_host_graph_get(self._h, out.ctypes.data, n.value, C.byref(n), inc.ctypes.data, C.byref(c)),
                "hc_host_graph_get")
        return out, inc, c.as_dict()

    def __del__(self):
        try:
            if self._h:
                N.lib.hc_host_graph_free(self._h)
        except Exception:
            pass


def keep_devices(on=True):
    """hc_ec_keep_devices: closed stages park their devices (contexts, text blocks, page-locked buffers) for the next one of this process."""
    N.check(N.lib.hc_ec_keep_devices(1 if on else 0), "hc_ec_keep_devices")


def fastq_on_device(on=True):
    """hc_ec_fastq_on_device: while on, a stage opened on one device with regular files reads its FASTQ files on the device
    (EdgeScorer.set_reads_from_fastq's call) and keeps no bases or qualities on the host.  Process-wide, off by default."""
    N.check(N.lib.hc_ec_fastq_on_device(1 if on else 0), "hc_ec_fastq_on_device")


def sam_on_device(on):
    """hc_ec_sam_on_device: off = every construct_edges_from_sam takes the host mirror's text route.  Process-wide, on by default."""
    N.check(N.lib.hc_ec_sam_on_device(1 if on else 0), "hc_ec_sam_on_device")


class EdgeCalculatorStage:
    """FastqStorage + OverlapGraph + EdgeCalculator, driven like src/ViralQuasispecies.cpp:233-283."""

    def __init__(self, settings: Settings, singles=None, paired1=None, paired2=None, ids=None, overlaps=None,
                 output_dir="", max_reads=0):
        self._h = _vp()
        self._cs = settings.to_c()
        self._paths = make_paths(singles, paired1, paired2, ids, overlaps, output_dir, max_reads)
        N.check(N.lib.hc_ec_open(C.byref(self._h), C.byref(self._cs), C.byref(self._paths)), "hc_ec_open")

    def construct_edges(self):
        N.check(N.lib.hc_ec_construct_edges(self._h), "hc_ec_construct_edges")

    def construct_edges_sorted(self):
        """construct_edges() + sortEdges() as one call (the lists arrive from the device in sortEdges order)."""
        N.check(N.lib.hc_ec_construct_edges_sorted(self._h), "hc_ec_construct_edges_sorted")

    def construct_edges_from_reads(self, err_rate, min_overlap, reversals=True, inclusions=True, sorted_order=True):
        """hc_ec_construct_edges_from_reads: candidates found on the device, ingested and scored without an overlaps file.
        Returns (SFO records found, overlap lines)."""
        nf, nl = C.c_uint64(), C.c_uint64()
        flags = (1 if reversals else 0) | (2 if inclusions else 0)
        N.check(N.lib.hc_ec_construct_edges_from_reads(self._h, float(err_rate), int(min_overlap), flags, 1 if sorted_order else 0,
                                                       C.byref(nf), C.byref(nl)), "hc_ec_construct_edges_from_reads")
        return nf.value, nl.value

    def construct_edges_from_sfo(self, sfo_path, sorted_order=True):
        """hc_ec_construct_edges_from_sfo: the SFO file rust-overlaps wrote -> graph (scripts/sfo2overlaps.py + the overlaps file + the text
        parser in one call; nothing but device memory in between for a canonical file).  Returns (SFO records, overlap lines, on_device)."""
        nr, nl, dr = C.c_uint64(), C.c_uint64(), C.c_int()
        N.check(N.lib.hc_ec_construct_edges_from_sfo(self._h, _b(sfo_path), 1 if sorted_order else 0, C.byref(nr), C.byref(nl), C.byref(dr)),
                "hc_ec_construct_edges_from_sfo")
        return nr.value, nl.value, bool(dr.value)

    def construct_edges_from_sam(self, sam_s, sam_p, ref_fasta, min_overlap_len=0, sorted_order=True):
        """hc_ec_construct_edges_from_sam: bwa's SAM files and the reference -> graph (scripts/sam2overlaps.py + the overlaps file + the text
        parser in one call; the lines are enumerated on the device and stay there).  Returns (records, overlap lines, on_device)."""
        nr, nl, dr = C.c_uint64(), C.c_uint64(), C.c_int()
        N.check(N.lib.hc_ec_construct_edges_from_sam(self._h, _b(sam_s), _b(sam_p), _b(ref_fasta), int(min_overlap_len), 1 if sorted_order else 0,
                                                     C.byref(nr), C.byref(nl), C.byref(dr)), "hc_ec_construct_edges_from_sam")
        return nr.value, nl.value, bool(dr.value)

    def construct_edges_from_store(self, err_rate, min_overlap, reversals=True, inclusions=True, sorted_order=True):
        """hc_ec_construct_edges_from_store: the same with nothing but device memory between the reads and the graph (no text is written,
        copied or parsed).  Returns (SFO records found, overlap lines, whether the lines stayed on the device)."""
        nf, nl, dr = C.c_uint64(), C.c_uint64(), C.c_int()
        flags = (1 if reversals else 0) | (2 if inclusions else 0)
        N.check(N.lib.hc_ec_construct_edges_from_store(self._h, float(err_rate), int(min_overlap), flags, 1 if sorted_order else 0,
                                                       C.byref(nf), C.byref(nl), C.byref(dr)), "hc_ec_construct_edges_from_store")
        return nf.value, nl.value, bool(dr.value)

    def device_count(self):
        return int(N.lib.hc_ec_device_count(self._h))

    def counters(self):
        c = hc_ec_counters()
        N.check(N.lib.hc_ec_get_counters(self._h, C.byref(c)), "hc_ec_get_counters")
        return c.as_dict()

    def read_count(self):
        return int(N.lib.hc_ec_read_count(self._h))

    def edge_count(self):
        return int(N.lib.hc_ec_edge_count(self._h))

    def edges(self):
        n = C.c_uint64()
        N.check(N.lib.hc_ec_get_edges(self._h, None, 0, C.byref(n)), "hc_ec_get_edges")
        out = np.zeros(n.value, dtype=EDGE_DTYPE)
        N.check(N.lib.hc_ec_get_edges(self._h, out.ctypes.data, n.value, C.byref(n)), "hc_ec_get_edges")
        return out

    def vertex_count(self):
        return int(N.lib.hc_ec_vertex_count(self._h))

    def inclusions(self):
        out = np.zeros(self.vertex_count(), np.uint8)
        N.check(N.lib.hc_ec_get_inclusions(self._h, out.ctypes.data, out.size), "hc_ec_get_inclusions")
        return out

    def fastq_was_on_device(self):
        """hc_ec_fastq_was_on_device: True when this stage's FASTQ files were read on the device (fastq_on_device)."""
        return bool(N.lib.hc_ec_fastq_was_on_device(self._h))

    def read_seq(self, index, mate=0, phred=False):
        """Read::get_seq / get_phred of read `index` (mate 0: a single-end read, 1 / 2: a pair's) as bytes."""
        n = C.c_uint64()
        N.check(N.lib.hc_ec_get_read_seq(self._h, int(index), int(mate), int(bool(phred)), None, 0, C.byref(n)), "hc_ec_get_read_seq")
        buf = C.create_string_buffer(max(1, n.value))
        N.check(N.lib.hc_ec_get_read_seq(self._h, int(index), int(mate), int(bool(phred)), buf, n.value, C.byref(n)), "hc_ec_get_read_seq")
        return buf.raw[:n.value]

    def sort_edges(self):
        """overlap_graph->sortEdges(), the call after construct_edges in src/ViralQuasispecies.cpp:297."""
        N.check(N.lib.hc_ec_sort_edges(self._h), "hc_ec_sort_edges")

    def in_lists(self):
        n = self.edge_count()
        off = np.zeros(self.vertex_count() + 1, np.uint64)
        nodes = np.zeros(max(n, 1), np.uint64)
        N.check(N.lib.hc_ec_get_in_lists(self._h, off.ctypes.data, nodes.ctypes.data, n), "hc_ec_get_in_lists")
        return off, nodes[:n]

    def overlap_score(self, seq1, seq2, phred1, phred2, pos):
        sc, mr = C.c_double(), C.c_double()
        N.check(N.lib.hc_ec_overlap_score(self._h, _b(seq1), _b(seq2), _b(phred1), _b(phred2), pos, C.byref(sc),
                                          C.byref(mr)), "hc_ec_overlap_score")
        return sc.value, mr.value

    def close(self):
        if self._h:
            N.lib.hc_ec_close(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sr_consensus(reads, layouts, members, min_qual=0.99, min_clique_size=2, error_correction=False, subreads_needed=False, n_threads=1):
    """hc_host_sr_consensus: the host mirror of EdgeScorer.sr_consensus on a ReadSet (SRBuilder::consensus, src/SRBuilder.cpp:289-535)."""
    from . import consensus as SR

    st = SR.make_settings(min_qual, min_clique_size, error_correction, subreads_needed, n_threads)

    def p(a):
        return a.ctypes.data if a.size else None

    return SR.run(lambda *a: N.lib.hc_host_sr_consensus(p(reads.bases), p(reads.quals), p(reads.seq_off), p(reads.read_first_seq), reads.n_reads, *a),
                  layouts, members, st)


def sr_merge_self_overlaps(seq, qual, pairs, settings=None, min_score=0.99, min_qual=0.99, min_overlap=15, n_threads=1, count_first=False):
    """hc_host_sr_merge_self_overlaps: the host mirror of EdgeScorer.sr_merge_self_overlaps (SRBuilder::merge_self_overlap,
    src/SRBuilder.cpp:872-955).  settings: a records.Settings, of which --mismatch and --min_read_len are read."""
    from . import consensus as SR
    from .records import Settings

    cs = (settings or Settings()).to_c()
    st = SR.make_self_settings(min_score, min_qual, min_overlap, n_threads)
    return SR.run_self(lambda *a: N.lib.hc_host_sr_merge_self_overlaps(C.byref(cs), *a), seq, qual, pairs, st, count_first)


def sr_edge_layouts(edges, reads):
    """hc_host_sr_edge_layouts: layouts of edge merges between single-end reads (sort_vertices type 's', src/SRBuilder.cpp:33-285)."""
    from . import consensus as SR

    return SR.edge_layouts(edges, reads)


def graph_merge_pairs(edges, out_off):
    """hc_host_graph_merge_pairs: OverlapGraph::getEdgesForMerging (src/GraphAlgos.cpp:112-148) on a caller's records; (n, 2) vertex ids."""
    from . import consensus as SR

    e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    oo = np.ascontiguousarray(out_off, dtype=np.uint64)
    return SR.merge_pairs(lambda p, cap, n: N.lib.hc_host_graph_merge_pairs(e.ctypes.data if e.size else None, oo.ctypes.data, oo.size - 1, p, cap, n),
                          oo.size - 1)


def sr_edge_merge_layouts(edges, out_off, reads, pairs, vertex_read, vertex_fwd, ret=None, min_clique_size=2):
    """hc_host_sr_edge_merge_layouts: the host mirror of EdgeScorer.sr_edge_merge's layouts and subread infos (sort_vertices and
    calcSubreadInfo, src/SRBuilder.cpp:33-285, 536-595).  ret: the layouts' consensus return values, for the subread infos."""
    from . import consensus as SR

    return SR.host_edge_merge_layouts(edges, out_off, reads, pairs, vertex_read, vertex_fwd, SR.make_settings(min_clique_size=min_clique_size), ret)


def sr_clique_merge_layouts(edges, out_off, reads, clique_off, clique_nodes, vertex_read, vertex_fwd, ret=None, min_clique_size=2):
    """hc_host_sr_clique_merge_layouts: the host mirror of EdgeScorer.sr_clique_merge's layouts, filter and subread infos (sort_vertices,
    filter_subreads and calcSubreadInfo, src/SRBuilder.cpp:33-285, 597-651, 536-595).  ret: the layouts' consensus return values."""
    from . import consensus as SR

    return SR.host_clique_merge_layouts(edges, out_off, reads, clique_off, clique_nodes, vertex_read, vertex_fwd,
                                        SR.make_settings(min_clique_size=min_clique_size), ret)


def sr_merge_next(reads, cons_seq, cons_qual, pairs, edge, vertex_read, vertex_fwd, **kw):
    """hc_host_sr_merge_next: the host mirror of EdgeScorer.sr_merge_next (process_cliques and mergeAlongEdges, src/SRBuilder.cpp:981-1001,
    1260-1380) on a ReadSet and the consensus bytes of the edge merge.  kw: merge_next.host_merge_next's further arguments."""
    from . import merge_next as MN

    return MN.host_merge_next(reads, cons_seq, cons_qual, pairs, edge, vertex_read, vertex_fwd, **kw)


def sr_clique_next(reads, cons_seq, cons_qual, clique_off, clique_nodes, merged, vertex_read, vertex_fwd, **kw):
    """hc_host_sr_clique_next: the host mirror of EdgeScorer.sr_clique_next (process_cliques and cliquesToSuperreads, src/SRBuilder.cpp:981-1001,
    1122-1233) on a ReadSet and the consensus bytes of the clique merge.  kw: clique_next.host_clique_next's further arguments."""
    from . import clique_next as CN

    return CN.host_clique_next(reads, cons_seq, cons_qual, clique_off, clique_nodes, merged, vertex_read, vertex_fwd, **kw)


def sr_clique_select(clique_off, clique_nodes, n_vertices, min_clique_size=2, remove_multi_occ=False):
    """hc_host_sr_clique_select: the gate in front of process_cliques (src/SRBuilder.cpp:1056-1084: remove_multi_occ, the singleton count,
    minCliqueSize) over a CSR of cliques in file order.  Returns a clique_next.CliqueSelection."""
    from . import clique_next as CN

    return CN.host_clique_select(clique_off, clique_nodes, n_vertices, min_clique_size, remove_multi_occ)


def graph_write_text(graph: HostGraph, kind, **kw):
    """hc_host_graph_write_text on a HostGraph: the mirror of Scorer.graph_write_text; (bytes, counts)."""
    return graph.write_text(kind, **kw)


def sr_originals_next(off, entries, res, merged=None, vertex_read=None, vertex_fwd=None, first_it=False, n_threads=1, cap=None):
    """hc_host_sr_originals_next: the host mirror of EdgeScorer.sr_originals_next (src/SRBuilder.cpp:750-806, :938-949, :1161-1216, :1312-1369)
    on the dict (off, entries) of the store the merge call found.  res: what sr_merge_next / sr_clique_next returned, or an originals.Tables."""
    from . import originals as OR

    t = res if isinstance(res, OR.Tables) else OR.tables_from(res, merged, vertex_read, vertex_fwd, first_it)
    return OR.host_next(off, entries, t, n_threads, cap)


def sr_originals_text(off, entries):
    """hc_host_sr_originals_text: the bytes of subreads.txt for a dict (the writers' loop, src/SRBuilder.cpp:1449-1463)."""
    from . import originals as OR

    return OR.host_text(off, entries)


def sr_originals_parse(data):
    """hc_host_sr_originals_parse: the bytes of a subreads.txt -> (off, entries), OverlapGraph::buildOriginalsDict's else branch
    (src/OverlapGraph.cpp:807-838)."""
    from . import originals as OR

    return OR.host_parse(data)


def fno3_from_originals(off, entries, reads, counts3, original_readcount, walk_rank=None, max_combos=0, flags=0):
    """hc_host_fno3_from_originals: the host mirror of EdgeScorer.fno3_from_originals on a dict (off, entries) and one fno.FNO_READ_DTYPE
    record per read (id: what the lines print)."""
    from . import originals as OR

    return OR.host_fno3_from_originals(off, entries, reads, counts3, original_readcount, walk_rank, max_combos, flags)


def sr_fastq_text(reads, file):
    """hc_host_sr_fastq_text: the bytes a ReadSet's reads put into singles.fastq (file 0), paired1.fastq (1) or paired2.fastq (2), in
    ascending id (src/SRBuilder.cpp:1434-1447, :1484-1487, :1528-1535)."""
    from . import fastq_text as FQ

    return FQ.host_fastq_text(reads, file)


def sr_fastq_tips_text(reads, tip_reads):
    """hc_host_sr_fastq_tips_text: the bytes of removed_tip_sequences.fastq for the reads tip_reads[k] of a ReadSet (writeTipsToFile,
    src/SRBuilder.cpp:1386-1414)."""
    from . import fastq_text as FQ

    return FQ.host_fastq_tips_text(reads, tip_reads)


def br_evidence(graph, reads, orig_off, entries, original_bases, original_seq_off, vertex_read, vertex_fwd, settings, n_threads=1):
    """hc_host_br_evidence: the host mirror of EdgeScorer.br_evidence + br_evidence_fetch (src/BranchReduction.cpp:229-743 for every branch,
    :60-80) on a graph as graph_fetch returns it, a ReadSet, the dict over its reads and the original reads -> branch_evidence.BranchEvidence."""
    from . import branch_evidence as BR

    return BR.host_evidence(graph, reads, orig_off, entries, original_bases, original_seq_off, vertex_read, vertex_fwd, settings, n_threads)


def br_reduce(graph, reads, evidence, settings):
    """hc_host_br_reduce: the host mirror of EdgeScorer.br_reduce (src/BranchReduction.cpp:82-227, :745-1272) on a graph as graph_fetch returns
    it, a ReadSet and a branch_evidence.BranchEvidence -> (BranchReduction, the reduced graph, the records appended to branching_edges)."""
    from . import branch_evidence as BR

    return BR.host_reduce(graph, reads, evidence, settings)
