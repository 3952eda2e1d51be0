"""ctypes bindings for libhcedge.so (include/hcedge.h).  Fails loudly if the library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
lib_path = os.path.join(_HERE, "csrc", "libhcedge.so")


class HcError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        try:
            msg = lib.hc_strerror(status).decode()
            detail = lib.hc_last_error().decode()
        except Exception:  # pragma: no cover
            msg, detail = "?", ""
        super().__init__(f"{where}: {msg} ({status}) {detail}".strip())


if not os.path.exists(lib_path):
    raise ImportError(
        f"{lib_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C haploconduct_amd/csrc`.  haploconduct_amd has no CPU fallback."
    )

# PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP runtimes in
# one process cannot both own the GPU, so when torch is installed let it load its runtime
# first: libhcedge.so (linked against libamdhip64.so.7 by SONAME) then binds to that copy.
try:  # pragma: no cover - depends on the environment
    import torch  # noqa: F401
except Exception:  # torch is optional for the C ABI itself
    pass

lib = C.CDLL(lib_path)


class hc_settings(C.Structure):
    _fields_ = [
        ("edge_threshold", C.c_double),
        ("ov_threshold", C.c_double),
        ("merge_contigs", C.c_double),
        ("mismatch", C.c_double),
        ("min_read_len", C.c_uint32),
        ("min_overlap_len", C.c_uint32),
        ("min_overlap_perc", C.c_uint32),
        ("flags", C.c_uint32),
        ("max_overlaps", C.c_uint64),
        ("device", C.c_int32),
        ("n_threads", C.c_uint32),
        ("device_mask", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hc_text_result(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_lines", "lines_read", "needs_host", "n_nonplain", "n_unknown_id", "self_overlaps", "silently_dropped",
                                          "prefilter_rejected", "scored")] + \
               [("rows", C.c_void_p), ("n_rows", C.c_uint64), ("rejected", C.c_void_p), ("n_rejected", C.c_uint64),
                ("nonplain", C.c_void_p), ("n_nonplain_listed", C.c_uint64)]


class hc_graph_counts(C.Structure):
    _fields_ = [("n_admitted", C.c_uint64), ("n_edges", C.c_uint64), ("inclusion_count", C.c_uint64), ("dup_count", C.c_uint64),
                ("n_tied_lists", C.c_uint64), ("first_bad", C.c_int64)]


class hc_clean_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("edges_before", "edges_after", "transitive_count", "del_count", "rebuilt", "n_tied_lists")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class hc_read_geom(C.Structure):
    _fields_ = [("len1", C.c_uint32), ("len2", C.c_uint32), ("paired", C.c_uint8), ("pad", C.c_uint8 * 3)]


class hc_tip_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("edges_before", "edges_after", "out_tip_count", "tip_count", "n_removed", "n_tip_reads")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class hc_branch_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("edges_before", "edges_after", "n_removed", "transitive_kept", "n_out_branch", "n_in_branch",
                                          "n_components", "n_tied_lists", "cc_rounds")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class hc_label_settings(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("n_reads", C.c_uint64)]


class hc_label_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("edges_before", "edges_after", "conflict_count", "n_moved", "n_switched", "tries", "best_try",
                                          "n_components", "n_inconsistent", "n_host_vertices", "n_host_edges")] + \
               [(k, C.c_uint32) for k in ("status", "bad_v", "bad_pos", "pad")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


LABEL_STATUS = ("OK", "DUPLICATE_EDGE", "REPEATED_RECORD")  # HC_LABEL_*


def label_settings(resolve_orientations=True, add_duplicates=False, n_reads=0):
    """hc_label_settings from the two switches (HC_FLAG_RESOLVE_ORIENTATIONS = 0x2, HC_FLAG_ADD_DUPLICATES = 0x1)."""
    return hc_label_settings((0x2 if resolve_orientations else 0) | (0x1 if add_duplicates else 0), int(n_reads))


class hc_graph_text_settings(C.Structure):
    _fields_ = [("edge_threshold", C.c_double), ("merge_contigs", C.c_double), ("n_singles", C.c_uint64)]


class hc_graph_text_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_bytes", "n_lines", "n_pairs", "n_segments", "l_count", "c_count")] + \
               [("status", C.c_uint32), ("pad", C.c_uint32), ("bad_v", C.c_uint64), ("bad_pos", C.c_uint64), ("ms_device", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


GRAPH_TEXT_KINDS = {"cliques": 0, "digraph": 1, "gfa": 2}  # HC_GRAPH_TEXT_*
GRAPH_TEXT_STATUS = ("OK", "SELF_LOOP", "INCLUSION_HAS_EDGES", "WEAK_EDGE", "PAIRED_IN_SINGLES", "EMPTY_SEQ", "BAD_BASE")


class hc_sr_settings(C.Structure):  # include/hcsr.h
    _fields_ = [("min_qual", C.c_double), ("min_clique_size", C.c_uint32), ("error_correction", C.c_uint32), ("subreads_needed", C.c_uint32),
                ("n_threads", C.c_uint32)]


class hc_sr_stats(C.Structure):
    _fields_ = [("n_columns", C.c_uint64), ("n_host_columns", C.c_uint64), ("ms_device", C.c_double), ("ms_host_finish", C.c_double)]


class hc_sr_clique_stats(C.Structure):
    _fields_ = [("sr", hc_sr_stats), ("n_filtered_layouts", C.c_uint64), ("n_host_filters", C.c_uint64), ("ms_layout", C.c_double),
                ("ms_host_filter", C.c_double)]


class hc_merge_pairs_stats(C.Structure):
    _fields_ = [("ms_kernel", C.c_double), ("ms_copy", C.c_double), ("ms_walk", C.c_double)]


class hc_sr_self_settings(C.Structure):
    _fields_ = [("min_score", C.c_double), ("min_qual", C.c_double), ("min_overlap", C.c_uint32), ("n_threads", C.c_uint32)]


class hc_sr_self_stats(C.Structure):
    _fields_ = [("n_merged", C.c_uint64), ("n_host_pairs", C.c_uint64), ("n_offsets", C.c_uint64), ("ms_device", C.c_double), ("ms_host", C.c_double)]


class hc_sr_next_settings(C.Structure):
    _fields_ = [("keep_singletons", C.c_uint32), ("reserved", C.c_uint32)]


class hc_sr_next_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_kept", "n_dropped_empty", "n_dropped_n_rate", "n_dropped_short", "n_bad", "n_seq", "n_bytes")] + \
               [("ms_device", C.c_double), ("ms_plan", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class hc_br_threshold(C.Structure):  # include/hcsr.h: hc_br_reduce
    _fields_ = [("dist", C.c_int32), ("min_evidence", C.c_int32)]


class hc_br_reduce_settings(C.Structure):
    _fields_ = [("careful", C.c_uint32), ("diploid", C.c_uint32), ("verbose", C.c_uint32), ("reserved", C.c_uint32), ("thresholds", C.c_void_p),
                ("n_thresholds", C.c_uint64)]


class hc_br_reduce_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_components", "n_component_edges", "n_false_dropped", "n_no_threshold", "n_careful_dropped", "n_kept", "n_removed",
                                          "n_missing_appended", "n_items_sorted", "n_host_finished")] + \
               [("ms_device", C.c_double), ("ms_host_walk", C.c_double), ("ms_copy", C.c_double), ("ms_sort", C.c_double), ("ms_edit", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class hc_br_reduce_tables(C.Structure):
    _fields_ = [("components", C.c_void_p), ("cap_components", C.c_uint64), ("comp_edge", C.c_void_p), ("comp_unique", C.c_void_p),
                ("cap_comp_edges", C.c_uint64), ("removed", C.c_void_p), ("cap_removed", C.c_uint64)]


class hc_br_host_graph_out(C.Structure):
    _fields_ = [("edges", C.c_void_p), ("cap_edges", C.c_uint64), ("out_off", C.c_void_p), ("in_nodes", C.c_void_p), ("in_off", C.c_void_p),
                ("branching", C.c_void_p), ("cap_branching", C.c_uint64), ("n_edges", C.c_uint64), ("n_branching", C.c_uint64)]


_vp = C.c_void_p
_u64p = C.POINTER(C.c_uint64)
_sr_tail = [_vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(hc_sr_settings), _vp, _vp, _vp, _vp, _vp, C.c_uint64, _u64p, C.POINTER(hc_sr_stats)]
_sr_self_tail = [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(hc_sr_self_settings), _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _u64p,
                 C.POINTER(hc_sr_self_stats)]
_sr_next_tail = [_vp, C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(hc_sr_next_settings), _vp, _vp, C.POINTER(hc_sr_next_counts)]
# hc_fno1_from_graph (include/hcsr.h): FNO=1 from the graph and the tables the context holds
FNO1_TABLES_CALLER, FNO1_TABLES_KEPT = 0, 1


class hc_fno1_resident_input(C.Structure):
    _fields_ = [("tables", C.c_uint32), ("flags", C.c_uint32), ("nodes", C.c_void_p), ("n_nodes", C.c_uint64), ("srs", C.c_void_p), ("n_srs", C.c_uint64),
                ("clique_off", C.c_void_p), ("clique_nodes", C.c_void_p), ("subread_off", C.c_void_p), ("subreads", C.c_void_p),
                ("nonedges", C.c_void_p), ("n_nonedges", C.c_uint64), ("new_read_count", C.c_uint64), ("edge_threshold", C.c_double),
                ("max_induced_pairs", C.c_uint64)]


class hc_fno1_resident_counts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_lines", "n_bytes", "copied", "u2sr", "v2sr", "sr2sr", "n_graph_edges", "n_branching", "n_nonedges_kept",
                                          "n_induced_pairs", "n_induced", "n_items")] + [("ms_device", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_sig = {
    "hc_sr_keep_device": (C.c_int, [_vp, C.c_int]),
    "hc_sr_set_next_reads": (C.c_int, [_vp] + _sr_next_tail),
    "hc_sr_next_reads_fetch": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p, _u64p, _u64p]),
    "hc_host_sr_next_reads": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint64] + _sr_next_tail + [_vp, _vp, C.c_uint64, _u64p, _vp, _vp]),
    "hc_sr_merge_self_overlaps": (C.c_int, [_vp] + _sr_self_tail),
    "hc_host_sr_merge_self_overlaps": (C.c_int, [C.POINTER(hc_settings)] + _sr_self_tail),
    "hc_sr_merge_self_overlaps_kept": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(hc_sr_self_settings), _vp, _vp, _vp, _vp, _u64p,
                                                 C.POINTER(hc_sr_self_stats)]),
    "hc_sr_kept_load": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "hc_sr_kept_fetch": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp, _vp, _u64p]),
    "hc_sr_consensus": (C.c_int, [_vp] + _sr_tail),
    "hc_host_sr_consensus": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32] + _sr_tail),
    "hc_host_sr_column": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, C.c_double, _vp]),
    "hc_host_sr_table": (C.c_int, [C.c_double, C.c_uint32, _vp]),
    "hc_host_sr_edge_layouts": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint32, _vp, _vp, _u64p]),
    "hc_graph_merge_pairs": (C.c_int, [_vp, _vp, C.c_uint64, _u64p, C.POINTER(hc_merge_pairs_stats)]),
    "hc_host_graph_merge_pairs": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _u64p]),
    "hc_sr_edge_merge": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(hc_sr_settings), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, C.c_uint64, _u64p, C.POINTER(hc_sr_stats)]),
    "hc_host_sr_edge_merge_layouts": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, C.POINTER(hc_sr_settings), _vp,
                                                _vp, _vp, _vp, _vp, _vp]),
    "hc_sr_clique_merge": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(hc_sr_settings), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, C.c_uint64, _u64p, C.POINTER(hc_sr_clique_stats)]),
    "hc_sr_clique_filter_on_host": (C.c_int, [_vp, C.c_int]),
    "hc_host_sr_clique_merge_layouts": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint64, _vp, _vp, C.POINTER(hc_sr_settings),
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(hc_sr_clique_stats)]),
    "hc_host_sr_clique_filter": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _vp, C.POINTER(C.c_uint32)]),
    "hc_version": (C.c_char_p, []),
    "hc_strerror": (C.c_char_p, [C.c_int]),
    "hc_last_error": (C.c_char_p, []),
    "hc_device_count": (C.c_int, []),
    "hc_create": (C.c_int, [C.POINTER(_vp), C.POINTER(hc_settings)]),
    "hc_destroy": (C.c_int, [_vp]),
    "hc_set_reads": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32]),
    "hc_score_batch": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "hc_score_batch_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),
    "hc_synchronize": (C.c_int, [_vp]),
    "hc_compact_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, _vp]),
    "hc_find_overlaps": (C.c_int, [_vp, C.c_double, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_found_to_overlaps": (C.c_int, [_vp, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_set_found_records": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_set_found_from_sfo_text": (C.c_int, [_vp, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_found_to_lines_device": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "hc_found_lines_fetch": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "hc_set_sam_records": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64]),
    "hc_sam_plan": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_uint64)]),
    "hc_sam_lines_device": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "hc_sam_lines_fetch": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "hc_sam_plan_counts": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hc_sam_lines_slot": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "hc_score_pack_device": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    "hc_narrow_payload_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),
    "hc_pack_cands": (None, [_vp, C.c_uint64, _vp]),
    "hc_score_cands": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "hc_score_cands_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),
    "hc_block_create": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    "hc_block_submit": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "hc_block_wait": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "hc_block_destroy": (C.c_int, [_vp]),
    "hc_text_set_ids": (C.c_int, [_vp, _vp, C.c_uint32]),
    "hc_textblock_create": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    "hc_textblock_buffer": (_vp, [_vp]),
    "hc_textblock_submit": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "hc_textblock_submit_lines": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "hc_textblock_submit_from": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64]),
    "hc_linechain_create": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    "hc_linechain_destroy": (C.c_int, [_vp]),
    "hc_textblock_wait": (C.c_int, [_vp, C.POINTER(hc_text_result)]),
    "hc_textblock_list_nonplain": (C.c_int, [_vp, C.c_uint32]),
    "hc_textblock_destroy": (C.c_int, [_vp]),
    "hc_textblock_regrown": (C.c_uint64, [_vp]),
    "hc_textblock_max_lines": (C.c_uint64, [_vp]),
    "hc_textblock_reserve_rows": (C.c_int, [_vp, C.c_uint64]),
    "hc_graph_begin": (C.c_int, [_vp]),
    "hc_graph_append": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_graph_resolve": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _vp, C.c_uint32, C.POINTER(hc_graph_counts)]),
    "hc_graph_fetch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hc_graph_size": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hc_graph_load": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, _vp]),
    "hc_graph_remove_inclusions": (C.c_int, [_vp, C.POINTER(hc_clean_counts)]),
    "hc_graph_remove_transitive": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(hc_clean_counts)]),
    "hc_graph_fetch_inclusion_edges": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hc_graph_remove_tips": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(hc_tip_counts)]),
    "hc_graph_remove_branches": (C.c_int, [_vp, C.POINTER(hc_branch_counts)]),
    "hc_graph_label_vertices": (C.c_int, [_vp, C.POINTER(hc_label_settings), C.POINTER(hc_label_counts)]),
    "hc_graph_fetch_orientations": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_graph_fetch_branching_edges": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_graph_fetch_tip_reads": (C.c_int, [_vp, _vp, C.c_uint64]),
    "hc_graph_write_text": (C.c_int, [_vp, C.c_uint32, C.POINTER(hc_graph_text_settings), C.POINTER(hc_graph_text_counts)]),
    "hc_graph_text_fetch": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "hc_reset": (C.c_int, [_vp, _vp]),
    "hc_set_comm_reserve": (C.c_int, [_vp, C.c_uint32]),
    "hc_comm_gate_device": (C.c_int, [_vp, _vp, C.c_uint32]),
    "hc_compact_pack_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    "hc_pack_rows_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    "hc_score_batch_compact": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_set_reorder": (C.c_int, [_vp, C.c_int]),
    "hc_host_alloc": (C.c_int, [_vp, C.POINTER(_vp), C.c_uint64]),
    "hc_host_free": (C.c_int, [_vp, _vp]),
    "hc_time_score_kernel": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, _vp, C.c_int, C.POINTER(C.c_float)]),
    "hc_count_positions_device": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hc_finalize": (C.c_int, [C.POINTER(hc_settings), _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "hc_finalize_batch": (C.c_int, [C.POINTER(hc_settings), _vp, C.c_uint64, _vp, _vp, _vp]),
    "hc_get_info": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)] + [C.POINTER(C.c_double)] * 4),
    "hc_get_kernel_info": (C.c_int, [_vp, C.c_char_p, C.c_uint32]),
    "hc_get_kernel_info_for": (C.c_int, [_vp, C.c_uint64, C.c_char_p, C.c_uint32]),
    "hc_get_locality_order": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hc_dev_radix_sort": (C.c_int, [C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint64, C.c_int, C.c_int]),
    "hc_dev_exclusive_sum": (C.c_int, [C.c_uint32, _vp, _vp, C.c_uint64]),
    "hc_dev_select_flagged": (C.c_int, [_vp, C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    "hc_dev_unique_u64": (C.c_int, [_vp, C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    "hc_fno1_from_graph": (C.c_int, [_vp, C.POINTER(hc_fno1_resident_input), C.POINTER(hc_fno1_resident_counts)]),
    "hc_fno1_text_fetch": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "hc_fno1_edges_fetch": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "hc_fno1_lines_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "hc_fno1_section_ms": (C.c_int, [_vp, C.POINTER(C.c_double * 4)]),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def check(status, where=""):
    if status != 0:
        raise HcError(status, where)


def device_count():
    return int(lib.hc_device_count())


def version():
    return lib.hc_version().decode()
