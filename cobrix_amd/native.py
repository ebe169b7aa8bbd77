"""ctypes binding of libcobrix_hip.so (include/cobrix_hip.h).

This is the Python counterpart of the JNI / Panama FFM stub a JVM host would use
(INTEGRATION.md).  There is no fallback: if the HIP library is missing, every product call
raises `NativeLibraryError`.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CBX_LIB_VARIANT=stamps selects the diagnostic build (tools/stamps.py); the product library otherwise
LIB_PATH = os.path.join(_HERE, "libcobrix_hip_%s.so" % os.environ["CBX_LIB_VARIANT"]
                        if os.environ.get("CBX_LIB_VARIANT") else "libcobrix_hip.so")

CBX_MAX_DIMS = 4
CBX_MAX_SEG_KEYS = 32
CBX_MAX_SEG_KEY_LEN = 32
CBX_MAX_SEG_LEVELS = 8
CBX_MAX_SEG_PREFIX = 64

# kinds / out types / flags (keep in sync with include/cobrix_hip.h)
K_STRING, K_STRING_ASCII, K_HEX, K_RAW, K_BCD, K_BINARY, K_ZONED = 1, 2, 3, 4, 5, 6, 7
K_ASCII_NUM, K_UTF16_BE, K_UTF16_LE = 8, 13, 14
K_FLOAT, K_DOUBLE, K_RECORD_ID, K_FILE_ID = 9, 10, 11, 12
O_I32, O_I64, O_DEC64, O_DEC128, O_F32, O_F64, O_STRING, O_BINARY = 1, 2, 3, 4, 5, 6, 7, 8
F_SIGNED, F_BIG_ENDIAN, F_EXPLICIT_DOT, F_INTEGRAL, F_IBM, F_LITTLE_ENDIAN_FP, F_DEPENDEE = (
    0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40)
F_LIST = 0x80
TRIM = {"none": 1, "left": 2, "right": 3, "both": 4}

CBX_OK, CBX_E_ARGUMENT, CBX_E_STATE, CBX_E_CAPACITY, CBX_E_HIP, CBX_E_UNSUPPORTED = 0, -1, -2, -3, -4, -5

OUT_WIDTH = {O_I32: 4, O_I64: 8, O_DEC64: 8, O_DEC128: 16, O_F32: 4, O_F64: 8}

# every symbol include/cobrix_hip.h declares
EXPORTED_SYMBOLS = ("cbx_abi_version", "cbx_last_error", "cbx_plan_create", "cbx_plan_destroy",
                    "cbx_string_bound", "cbx_string_view_geometry", "cbx_string_sizes_fixed", "cbx_decode_fixed", "cbx_decode_var",
                    "cbx_string_sizes_var", "cbx_plan_check", "cbx_frame_rdw", "cbx_frame_rdw_async", "cbx_frame_rdw_state",
                    "cbx_plan_set_profiling",
                    "cbx_plan_kernel_times", "cbx_plan_kernel_kind", "cbx_plan_frame_kind", "cbx_plan_specialize", "cbx_frame_text",
                    "cbx_sparse_index", "cbx_select_records", "cbx_decode_selected", "cbx_hier_select",
                    "cbx_hier_list_offsets", "cbx_plan_set_walk", "cbx_frame_var_occurs",
                    "cbx_plan_set_record_base", "cbx_frame_length_field", "cbx_plan_set_odo_counts",
                    "cbx_hier_dependee_counts", "cbx_hier_dependee_values", "cbx_plan_set_dep_seed", "cbx_views_to_utf8", "cbx_plan_pipeline",
                    "cbx_filter_records", "cbx_filter_pass_times", "cbx_plan_direct_eligible", "cbx_plan_launch_info", "cbx_plan_walk_info",
                    "cbx_aggregate_records", "cbx_aggregate_pass_times",
                    "cbx_group_layout", "cbx_aggregate_grouped", "cbx_group_pass_times",
                    "cbx_top_n_records", "cbx_top_n_info", "cbx_top_n_pass_times",
                    "cbx_key_set_create", "cbx_key_set_info", "cbx_key_set_destroy", "cbx_filter_records_keyed",
                    "cbx_key_set_create_from_records",
                    "cbx_filter_max_op",
                    "cbx_key_map_create_from_records", "cbx_key_map_info", "cbx_key_map_destroy", "cbx_key_map_set",
                    "cbx_join_records", "cbx_select_ordinals", "cbx_join_pass_times",
                    "cbx_key_map_index_rows", "cbx_key_map_rows_info", "cbx_key_map_rows", "cbx_join_records_expand",
                    "cbx_join_expand_info", "cbx_join_expand_pass_times")
# grouped aggregates were an additive extension of ABI 24: the symbols are required
GROUP_SYMBOLS = ("cbx_group_layout", "cbx_aggregate_grouped", "cbx_group_pass_times")
# Top-N / LIMIT pushdown was an additive extension of ABI 25: the symbols are required
TOPN_SYMBOLS = ("cbx_top_n_records", "cbx_top_n_info", "cbx_top_n_pass_times")
# key-set filters were an additive extension of ABI 25: the symbols are required
KEYSET_SYMBOLS = ("cbx_key_set_create", "cbx_key_set_info", "cbx_key_set_destroy", "cbx_filter_records_keyed")
# key sets built from a second file's records were an additive extension of ABI 25: the symbol is required
KEYSET_FROM_SYMBOLS = ("cbx_key_set_create_from_records",)
# suffix / substring filter ops were an additive extension of ABI 25: the symbol is required
FILTER_STRING_SYMBOLS = ("cbx_filter_max_op",)
# lookup joins (key maps, the join stage, rows by ordinal) were an additive extension of ABI 25: the symbols are required
KEYMAP_SYMBOLS = ("cbx_key_map_create_from_records", "cbx_key_map_info", "cbx_key_map_destroy", "cbx_key_map_set",
                  "cbx_join_records", "cbx_select_ordinals", "cbx_join_pass_times")
# fan-out joins (row lists on a key map, the expanding join stage) were an additive extension of ABI 25: the symbols
# are required
FANOUT_SYMBOLS = ("cbx_key_map_index_rows", "cbx_key_map_rows_info", "cbx_key_map_rows", "cbx_join_records_expand",
                  "cbx_join_expand_info", "cbx_join_expand_pass_times")
ABI_VERSION = 25


class NativeLibraryError(RuntimeError):
    pass


class CbxError(RuntimeError):
    """Structural error reported by the library (IllegalArgument/IllegalState in the reference)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"cbx error {code}: {msg}")
        self.code = code


class CbxField(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("out_type", ctypes.c_int32), ("offset", ctypes.c_int32),
                ("size", ctypes.c_int32), ("precision", ctypes.c_int32), ("scale", ctypes.c_int32),
                ("scale_factor", ctypes.c_int32), ("out_precision", ctypes.c_int32),
                ("out_scale", ctypes.c_int32), ("flags", ctypes.c_int32), ("trim", ctypes.c_int32),
                ("n_dims", ctypes.c_int32), ("dim_count", ctypes.c_int32 * CBX_MAX_DIMS),
                ("dim_stride", ctypes.c_int32 * CBX_MAX_DIMS), ("dim_array", ctypes.c_int32 * CBX_MAX_DIMS),
                ("segment", ctypes.c_int32), ("column", ctypes.c_int32)]


class CbxArray(ctypes.Structure):
    _fields_ = [("max_count", ctypes.c_int32), ("min_count", ctypes.c_int32), ("dependee", ctypes.c_int32),
                ("segment", ctypes.c_int32), ("count_column", ctypes.c_int32), ("n_dims", ctypes.c_int32),
                ("parent", ctypes.c_int32), ("offsets_column", ctypes.c_int32)]


class CbxSegmentMap(ctypes.Structure):
    _fields_ = [("field_offset", ctypes.c_int32), ("field_size", ctypes.c_int32), ("n_keys", ctypes.c_int32),
                ("key_len", ctypes.c_int32 * CBX_MAX_SEG_KEYS),
                ("key", (ctypes.c_uint16 * CBX_MAX_SEG_KEY_LEN) * CBX_MAX_SEG_KEYS),
                ("key_segment", ctypes.c_int32 * CBX_MAX_SEG_KEYS),
                ("key_level", ctypes.c_int32 * CBX_MAX_SEG_KEYS),
                ("key_in_filter", ctypes.c_int32 * CBX_MAX_SEG_KEYS),
                ("key_is_int", ctypes.c_int32 * CBX_MAX_SEG_KEYS),
                ("key_int", ctypes.c_int64 * CBX_MAX_SEG_KEYS),
                ("field", ctypes.c_int32), ("field_is_int", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("has_filter", ctypes.c_int32), ("level_column", ctypes.c_int32 * CBX_MAX_SEG_LEVELS),
                ("prefix_len", ctypes.c_int32), ("prefix", ctypes.c_uint8 * CBX_MAX_SEG_PREFIX)]


class CbxPlanOptions(ctypes.Structure):
    _fields_ = [("n_columns", ctypes.c_int32), ("file_id", ctypes.c_int32), ("has_segments", ctypes.c_int32),
                ("window_bytes", ctypes.c_int32), ("segment_column", ctypes.c_int32),
                ("jit_min_records", ctypes.c_int32), ("string_views", ctypes.c_int32), ("direct_decode", ctypes.c_int32),
                ("lut", ctypes.c_uint32 * 256),
                ("segments", CbxSegmentMap)]


class CbxColumn(ctypes.Structure):
    _fields_ = [("values", ctypes.c_void_p), ("validity", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("data", ctypes.c_void_p), ("data_capacity", ctypes.c_int64), ("data_sizes", ctypes.c_void_p)]


class CbxRdwParams(ctypes.Structure):
    _fields_ = [("big_endian", ctypes.c_int32), ("adjustment", ctypes.c_int32),
                ("file_header_bytes", ctypes.c_int32), ("file_footer_bytes", ctypes.c_int32)]


class CbxIndexEntry(ctypes.Structure):
    _fields_ = [("offset_from", ctypes.c_int64), ("offset_to", ctypes.c_int64), ("record_index", ctypes.c_int64),
                ("file_id", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CbxIndexParams(ctypes.Structure):
    _fields_ = [("records_per_entry", ctypes.c_int64), ("bytes_per_entry", ctypes.c_int64),
                ("subtract_size", ctypes.c_int32), ("header_bytes", ctypes.c_int32),
                ("has_file_header", ctypes.c_int32), ("hierarchical", ctypes.c_int32),
                ("file_id", ctypes.c_int32), ("reserved", ctypes.c_int32), ("start_bytes", ctypes.c_int64)]


class CbxSelection(ctypes.Structure):
    _fields_ = [("rec_off", ctypes.c_void_p), ("rec_len", ctypes.c_void_p), ("record_id", ctypes.c_void_p),
                ("segment", ctypes.c_void_p), ("seg_state", ctypes.c_void_p), ("file_id", ctypes.c_int32),
                ("footer_bytes", ctypes.c_int32)]


# row filters (cbx_filter): ops, table limits
(OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_IN, OP_NOT_IN, OP_IS_NULL, OP_IS_NOT_NULL, OP_STARTS_WITH,
 OP_NOT_STARTS_WITH, OP_ENDS_WITH, OP_NOT_ENDS_WITH, OP_CONTAINS, OP_NOT_CONTAINS) = range(1, 17)
FILTER_MAX_OP = OP_NOT_CONTAINS   # what cbx_filter_max_op answers
CBX_FILTER_MAX_TERMS, CBX_FILTER_MAX_LITERALS, CBX_FILTER_POOL_BYTES = 32, 64, 1024
# the filter stage keeps one count per tile of 64 records and scans them in blocks of kScanTile counts
# (cbx_kernels.hip: kScanBlock * kScanItems): a batch past FILTER_SCAN_BLOCK_RECORDS takes a second scan block
FILTER_TILE_RECORDS = 64
FILTER_SCAN_BLOCK_RECORDS = 256 * 8 * FILTER_TILE_RECORDS


class CbxFilterLiteral(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64), ("str_off", ctypes.c_int32),
                ("str_len", ctypes.c_int32)]


class CbxFilterTerm(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int32), ("op", ctypes.c_int32), ("group", ctypes.c_int32),
                ("lit_begin", ctypes.c_int32), ("lit_count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CbxFilter(ctypes.Structure):
    _fields_ = [("n_terms", ctypes.c_int32), ("n_literals", ctypes.c_int32), ("pool_bytes", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("terms", CbxFilterTerm * CBX_FILTER_MAX_TERMS),
                ("literals", CbxFilterLiteral * CBX_FILTER_MAX_LITERALS),
                ("pool", ctypes.c_uint8 * CBX_FILTER_POOL_BYTES)]


# aggregate pushdown (cbx_aggregate): function bits, table limit
AGG_COUNT, AGG_MIN, AGG_MAX, AGG_SUM = 1, 2, 4, 8
CBX_AGG_MAX_TERMS = 16


class CbxAggregateTerm(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int32), ("funcs", ctypes.c_int32)]


class CbxAggregate(ctypes.Structure):
    _fields_ = [("n_terms", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("terms", CbxAggregateTerm * CBX_AGG_MAX_TERMS)]


class CbxAggregateValue(ctypes.Structure):
    _fields_ = [("count", ctypes.c_int64), ("min_lo", ctypes.c_uint64), ("min_hi", ctypes.c_uint64),
                ("max_lo", ctypes.c_uint64), ("max_hi", ctypes.c_uint64), ("sum", ctypes.c_uint64 * 3)]


class CbxAggregateResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("values", CbxAggregateValue * CBX_AGG_MAX_TERMS)]


# grouped aggregates (cbx_group_by): key limit, workspace limit
CBX_GROUP_MAX_KEYS = 4
CBX_GROUP_MAX_WORKSPACE_BYTES = 1 << 30
GROUP_MAX_STRING_KEY_BYTES = 32


class CbxGroupBy(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_int32), ("fields", ctypes.c_int32 * CBX_GROUP_MAX_KEYS),
                ("reserved", ctypes.c_int32 * 3)]


class CbxGroupKey(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64), ("is_null", ctypes.c_int32),
                ("str_len", ctypes.c_int32)]


class CbxGroupStrides(ctypes.Structure):
    _fields_ = [("str_stride", ctypes.c_int32), ("str_off", ctypes.c_int32 * CBX_GROUP_MAX_KEYS),
                ("reserved", ctypes.c_int32 * 3), ("capacity", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)]


class CbxGroupOutput(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_void_p), ("values", ctypes.c_void_p), ("keys", ctypes.c_void_p),
                ("key_bytes", ctypes.c_void_p)]


class CbxGroupHeader(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("overflow", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


# Top-N (cbx_sort_order): key limit, flag bits
CBX_TOPN_MAX_KEYS = 4
SORT_DESC, SORT_NULLS_LAST = 1, 2


class CbxSortKey(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int32), ("flags", ctypes.c_int32)]


class CbxSortOrder(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_int32), ("reserved", ctypes.c_int32), ("keys", CbxSortKey * CBX_TOPN_MAX_KEYS)]


class CbxTopnInfo(ctypes.Structure):
    """cbx_top_n_info: how the plan's last Top-N call ran."""
    _fields_ = [("n_live", ctypes.c_int64), ("ties_after_level0", ctypes.c_int64), ("ties_max", ctypes.c_int64),
                ("grid", ctypes.c_int64), ("levels_run", ctypes.c_int32), ("levels_total", ctypes.c_int32),
                ("words_per_key", ctypes.c_int32 * CBX_TOPN_MAX_KEYS)]


# key sets (cbx_key_set): at most CBX_GROUP_MAX_KEYS key columns, at most CBX_GROUP_MAX_KEYS sets per keyed filter call
CBX_KEYSET_MAX_SETS = CBX_GROUP_MAX_KEYS


class CbxKeyValue(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64), ("str_len", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class CbxKeysetInfo(ctypes.Structure):
    """cbx_key_set_info: what the build of a key set found."""
    _fields_ = [("n_values", ctypes.c_int64), ("n_distinct", ctypes.c_int64), ("capacity", ctypes.c_int64),
                ("device_bytes", ctypes.c_int64), ("max_probe", ctypes.c_int64), ("build_ms", ctypes.c_float),
                ("n_keys", ctypes.c_int32)]


class CbxKeysetSourceInfo(ctypes.Structure):
    """cbx_key_set_create_from_records: what the pass over the source records found."""
    _fields_ = [("n_rows", ctypes.c_int64), ("n_null_rows", ctypes.c_int64), ("n_source_keys", ctypes.c_int64),
                ("n_dropped", ctypes.c_int64), ("source_capacity", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64),
                ("overflow", ctypes.c_int32), ("reserved", ctypes.c_int32), ("distinct_ms", ctypes.c_float),
                ("convert_ms", ctypes.c_float)]


class CbxKeymapInfo(ctypes.Structure):
    """cbx_key_map_info: cbx_keyset_source_info's fields, then what the fill pass found."""
    _fields_ = CbxKeysetSourceInfo._fields_ + [("n_duplicate_keys", ctypes.c_int64), ("max_rows_per_key", ctypes.c_int64),
                                               ("fill_ms", ctypes.c_float), ("reserved2", ctypes.c_int32)]


JOIN_INNER, JOIN_LEFT = 0, 1


class CbxKeymapRowsInfo(ctypes.Structure):
    """cbx_key_map_rows_info: the row lists of a key map and how their sort ran."""
    _fields_ = [("n_indexed_rows", ctypes.c_int64), ("n_short", ctypes.c_int64), ("n_lds", ctypes.c_int64),
                ("n_global", ctypes.c_int64), ("has_rows", ctypes.c_int32), ("short_max", ctypes.c_int32),
                ("lds_max", ctypes.c_int32), ("index_ms", ctypes.c_float)]


class CbxJoinExpandInfo(ctypes.Structure):
    """cbx_join_expand_info: how the last cbx_join_records_expand call ran."""
    _fields_ = [("n_kept", ctypes.c_int64), ("n_out", ctypes.c_int64), ("max_fanout", ctypes.c_int64),
                ("emit_grid", ctypes.c_int64), ("outputs_per_workgroup", ctypes.c_int32), ("host_waits", ctypes.c_int32)]


W_GROUP, W_PRIM = 0, 1
W_REDEFINED, W_REDEFINES = 0x1, 0x2


class CbxWalkNode(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "next", "child", "field", "array", "flags", "data_size",
                                                "actual_size", "segment", "dep_slot")]


class CbxWalkArray(ctypes.Structure):
    _fields_ = [("dep_slot", ctypes.c_int32), ("h_begin", ctypes.c_int32), ("h_end", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class CbxWalkHandler(ctypes.Structure):
    _fields_ = [("key_id", ctypes.c_int32), ("key_len", ctypes.c_int32), ("value", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("key", ctypes.c_uint8 * 64)]


class CbxHierParams(ctypes.Structure):
    _fields_ = [("n_segments", ctypes.c_int32), ("root_segment", ctypes.c_int32),
                ("parent", ctypes.c_int32 * CBX_MAX_SEG_KEYS), ("first_record_id", ctypes.c_int64),
                ("start_offset", ctypes.c_int32), ("flags", ctypes.c_int32), ("row_capacity", ctypes.c_int64)]


CBX_HIER_MAX_SEG, CBX_HIER_MAX_EVENTS, CBX_HIER_MAX_DEPS = 16, 32, 16
HIER_EVENT_END = -32768


class CbxHierDependee(ctypes.Structure):
    _fields_ = [("values", ctypes.c_void_p), ("validity", ctypes.c_void_p), ("out_type", ctypes.c_int32),
                ("walk_slot", ctypes.c_int32)]


class CbxHierOdoArray(ctypes.Structure):
    _fields_ = [("dependee", ctypes.c_int32), ("out_row", ctypes.c_int32), ("min_count", ctypes.c_int32),
                ("max_count", ctypes.c_int32), ("first_counts", ctypes.c_void_p)]


class CbxHierWalk(ctypes.Structure):
    _fields_ = [("n_segments", ctypes.c_int32), ("root_segment", ctypes.c_int32),
                ("table_base", ctypes.c_int64 * (CBX_HIER_MAX_SEG + 1)),
                ("table_rows", ctypes.c_int64 * (CBX_HIER_MAX_SEG + 1)),
                ("child_offsets", ctypes.c_void_p * CBX_HIER_MAX_SEG),
                ("children", (ctypes.c_int8 * CBX_HIER_MAX_SEG) * CBX_HIER_MAX_SEG),
                ("events", (ctypes.c_int16 * CBX_HIER_MAX_EVENTS) * (CBX_HIER_MAX_SEG + 1)),
                ("seeds", ctypes.c_void_p)]


STAGING_WINDOWED, STAGING_CONTIGUOUS, STAGING_SPAN = 0, 1, 2


class CbxLaunchInfo(ctypes.Structure):
    """cbx_plan_launch_info: how the plan's last decode call launched its decode kernel."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "staging", "coop", "kp", "padded_rows", "n_windows",
                                                "global_window", "count_kernel", "base_shift", "reserved")] + \
               [("grid", ctypes.c_int64), ("blocks_needed", ctypes.c_int64)]


def launch_info(plan_handle) -> CbxLaunchInfo:
    info = CbxLaunchInfo()
    check(load().cbx_plan_launch_info(plan_handle, ctypes.byref(info)))
    return info


class CbxWalkInfo(ctypes.Structure):
    """cbx_plan_walk_info: how the plan's last decode call launched the record walk."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "stage_cap", "vlds", "wave_lds", "depth", "stack_lds",
                                                "n_vslots", "n_sslots")] + \
               [("grid", ctypes.c_int64), ("n_tiles", ctypes.c_int64)]


def walk_info(plan_handle) -> CbxWalkInfo:
    info = CbxWalkInfo()
    check(load().cbx_plan_walk_info(plan_handle, ctypes.byref(info)))
    return info


_lib = None


def lib_path() -> str:
    return LIB_PATH


def load():
    """Load the HIP library; raises NativeLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.cbx_abi_version.restype = i32
    L.cbx_last_error.restype = ctypes.c_char_p
    L.cbx_plan_create.argtypes = [P, i32, P, i32, P, ctypes.POINTER(P)]
    L.cbx_plan_destroy.argtypes = [P]
    L.cbx_plan_destroy.restype = None
    L.cbx_string_bound.argtypes = [P, i64, P]
    L.cbx_string_view_geometry.argtypes = [P, P, P]
    L.cbx_string_sizes_fixed.argtypes = [P, P, i64, i32, i32, P, P]
    L.cbx_plan_check.argtypes = [P, P]
    L.cbx_decode_fixed.argtypes = [P, P, i64, i32, i32, i64, P, P]
    L.cbx_decode_var.argtypes = [P, P, i64, P, P, i64, i32, i64, P, P]
    L.cbx_string_sizes_var.argtypes = [P, P, i64, P, P, i64, i32, P, P]
    L.cbx_frame_rdw.argtypes = [P, i64, P, i32, P, P, P, i64, P, P]
    L.cbx_frame_rdw_async.argtypes = [P, i64, P, i32, P, P, P, i64, P, i32, P]
    L.cbx_frame_rdw_state.argtypes = [P, P, P]
    L.cbx_frame_text.argtypes = [P, i64, i32, P, P, i64, P, P, P]
    L.cbx_plan_set_profiling.argtypes = [P, i32]
    L.cbx_plan_kernel_times.argtypes = [P, P, P, i32, P]
    L.cbx_plan_kernel_kind.argtypes = [P, P]
    L.cbx_plan_frame_kind.argtypes = [P, P]
    L.cbx_plan_specialize.argtypes = [P, P, i64, P, i32]
    L.cbx_sparse_index.argtypes = [P, P, i64, P, P, i64, P, P, i64, P, P]
    L.cbx_select_records.argtypes = [P, P, i64, P, P, i64, i32, P, i32, P, P, P]
    L.cbx_decode_selected.argtypes = [P, P, i64, P, i64, i32, P, P]
    for name, at in (("cbx_hier_select", [P, P, i64, P, P, i64, P, P, P, P, P, P]),
                     ("cbx_hier_list_offsets", [P, i64, i64, i64, i64, P, P]),
                     ("cbx_plan_set_walk", [P, P, i32, i32, P, P, i32, i32]),
                     ("cbx_frame_var_occurs", [P, P, i64, i64, P, P, i64, P, P, P]),
                     ("cbx_plan_set_record_base", [P, P]),
                     ("cbx_frame_length_field", [P, P, i64, i32, i32, i32, i32, P, P, i64, P, P]),
                     ("cbx_plan_set_odo_counts", [P, P, i64]),
                     ("cbx_hier_dependee_counts", [P, P, i32, P, i32, P, i64, P, P]),
                     ("cbx_hier_dependee_values", [P, P, i64, P, P, i64, i32, i32, P, P, P]),
                     ("cbx_plan_set_dep_seed", [P, P, i64, i32]),
                     ("cbx_views_to_utf8", [P, i64, P, i64, P, P, i64, P, P]),
                     ("cbx_plan_pipeline", [P, P, i32, i32]),
                     ("cbx_filter_records", [P, P, i64, P, P, P, i64, i32, i32, i64, P, P, P, P]),
                     ("cbx_filter_pass_times", [P, P, P, P]),
                     ("cbx_plan_direct_eligible", [P, P]),
                     ("cbx_plan_launch_info", [P, P]),
                     ("cbx_plan_walk_info", [P, P]),
                     ("cbx_aggregate_records", [P, P, i64, P, P, P, i64, i32, i32, P, P, i32, P, P]),
                     ("cbx_aggregate_pass_times", [P, P, P]),
                     ("cbx_group_layout", [P, P, P, i64, P]),
                     ("cbx_aggregate_grouped", [P, P, i64, P, P, P, i64, i32, i32, P, P, P, i64, i32, P, P, P]),
                     ("cbx_group_pass_times", [P, P, P, P]),
                     ("cbx_top_n_records", [P, P, i64, P, P, P, i64, i32, i32, i64, P, P, i64, i32, P, P, P]),
                     ("cbx_top_n_info", [P, P]),
                     ("cbx_top_n_pass_times", [P, P, P, P]),
                     ("cbx_key_set_create", [P, P, P, P, i32, P, i64, P, ctypes.POINTER(P)]),
                     ("cbx_key_set_info", [P, P]),
                     ("cbx_key_set_destroy", [P]),
                     ("cbx_filter_records_keyed", [P, P, i64, P, P, P, i64, i32, i32, i64, P, P, P, i32, P, P, P]),
                     ("cbx_key_set_create_from_records", [P, P, P, P, P, i64, P, P, P, i64, i32, i32, P, i64, i32, P,
                                                          ctypes.POINTER(P), P]),
                     ("cbx_key_map_create_from_records", [P, P, P, P, P, i64, P, P, P, i64, i32, i32, P, i64, i32, P,
                                                          ctypes.POINTER(P), P]),
                     ("cbx_key_map_info", [P, P]),
                     ("cbx_key_map_destroy", [P]),
                     ("cbx_key_map_set", [P]),
                     ("cbx_join_records", [P, P, i64, P, P, P, i64, i32, i32, i64, P, P, P, i32, P, i32, P, P, P, P, P]),
                     ("cbx_select_ordinals", [P, P, i64, P, P, P, i64, i32, i32, i64, P, i64, P, P]),
                     ("cbx_join_pass_times", [P, P, P, P]),
                     ("cbx_key_map_index_rows", [P, P, P, P, i64, P, P, P, i64, i32, i32, P, i32, P, P]),
                     ("cbx_key_map_rows_info", [P, P]),
                     ("cbx_key_map_rows", [P, P, P]),
                     ("cbx_join_records_expand", [P, P, i64, P, P, P, i64, i32, i32, i64, P, P, P, i32, P, i32, P, i64, P, P,
                                                  P, P, P]),
                     ("cbx_join_expand_info", [P, P]),
                     ("cbx_join_expand_pass_times", [P, P, P, P])):
        if hasattr(L, name):   # (diagnostic builds of older revisions lack the newest entry points)
            getattr(L, name).argtypes = at
    if L.cbx_abi_version() != ABI_VERSION and not os.environ.get("CBX_LIB_VARIANT"):
        # (a diagnostic variant built from an older revision -- tools/build_variant.py -- is timed on the
        # entry points both revisions share)
        raise NativeLibraryError(f"{LIB_PATH}: ABI {L.cbx_abi_version()} != {ABI_VERSION}; rebuild it")
    missing = [n for n in GROUP_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (grouped aggregates); rebuild it")
    missing = [n for n in TOPN_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (Top-N pushdown); rebuild it")
    missing = [n for n in KEYSET_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (key-set filters); rebuild it")
    missing = [n for n in KEYSET_FROM_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (key sets from records); rebuild it")
    missing = [n for n in FILTER_STRING_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (suffix / substring filter ops); rebuild it")
    missing = [n for n in KEYMAP_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (lookup joins); rebuild it")
    missing = [n for n in FANOUT_SYMBOLS if not hasattr(L, n)]
    if missing and not os.environ.get("CBX_LIB_VARIANT"):
        raise NativeLibraryError(f"{LIB_PATH}: ABI {ABI_VERSION} without {', '.join(missing)} (fan-out joins); rebuild it")
    if hasattr(L, "cbx_key_set_destroy"):
        L.cbx_key_set_destroy.restype = None
    if hasattr(L, "cbx_key_map_destroy"):
        L.cbx_key_map_destroy.restype = None
        L.cbx_key_map_set.restype = P
    if hasattr(L, "cbx_filter_max_op"):
        L.cbx_filter_max_op.argtypes = []
        L.cbx_filter_max_op.restype = i32
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != CBX_OK:
        raise CbxError(rc, load().cbx_last_error().decode(errors="replace"))
