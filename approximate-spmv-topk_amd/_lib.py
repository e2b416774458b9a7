"""ctypes binding of the C ABI declared in include/tkspmv.h (libtkspmv.so, built in-tree by `make`).

There is no Python/CPU fallback: if the shared library is missing the import fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TKSPMV_LIB") or os.path.join(_HERE, "libtkspmv.so")  # TKSPMV_LIB: tuning builds

OK, ERR_INVALID, ERR_NOT_SORTED, ERR_DEVICE, ERR_NOMEM, ERR_IO, ERR_UNSUPPORTED, ERR_STATE = range(8)
F32, Q1_7, Q1_7_WIDE, F16, FIXED, Q1_7_F32 = 0, 1, 2, 3, 4, 5
IMPL_STREAM, IMPL_ROW_PER_LANE, IMPL_SCORES_SELECT = 0, 1, 2
MAX_COLS = 16384
MAX_K = 1024
CURSOR_START, CURSOR_AFTER, CURSOR_END = 0, 1, 2  # tkspmv_cursor.state
ROW_NNZ, ROW_L1, ROW_L2SQ, ROW_INV_L2 = 0, 1, 2, 3  # TKSPMV_ROW_*: the kinds of tkspmv_enqueue_row_stats
COL_NNZ, COL_MAX, COL_MIN = 0, 1, 2  # TKSPMV_COL_*: the kinds of tkspmv_enqueue_col_stats
NEAREST_MAX_N, NEAREST_NONE = 4, 0xFFFFFFFF  # TKSPMV_NEAREST_*: the longest list of tkspmv_enqueue_nearest and its "no vector" label
SUMS_RAW, SUMS_FLOAT, SUMS_UNIT = 0, 1, 2  # TKSPMV_SUMS_*: the modes of tkspmv_enqueue_label_sums ...
SUMS_ACCUMULATE, SUMS_SINK_LDS, SUMS_SINK_DIRECT = 1, 2, 4  # ... and its flags


class TkspmvError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"tkspmv error {status}: {message}")
        self.status = status
        self.message = message


class Desc(C.Structure):
    _fields_ = [
        ("rows", C.c_uint32), ("cols", C.c_uint32), ("nnz", C.c_uint64),
        ("row", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_float)),
        ("k", C.c_int32), ("partitions", C.c_int32), ("k_per_partition", C.c_int32), ("precision", C.c_int32),
        ("device", C.c_int32), ("first_row", C.c_uint32), ("min_score", C.c_float),
        ("waves_per_cu", C.c_int32), ("threads_per_wg", C.c_int32), ("nnz_per_lane", C.c_int32),
        ("stream_replicas", C.c_int32), ("fixed_width", C.c_int32), ("multi_q", C.c_int32), ("impl", C.c_int32), ("reserved", C.c_int32 * 1),
    ]


class Info(C.Structure):
    _fields_ = [
        ("rows", C.c_uint32), ("cols", C.c_uint32), ("nnz", C.c_uint64), ("packed_entries", C.c_uint64),
        ("packed_bytes", C.c_uint64), ("algorithmic_bytes", C.c_uint64), ("n_packets", C.c_uint32),
        ("packet_entries", C.c_uint32), ("n_wave_partitions", C.c_uint32), ("packets_per_partition", C.c_uint32),
        ("grid", C.c_uint32), ("block", C.c_uint32), ("n_groups", C.c_uint32), ("lds_bytes", C.c_uint32),
        ("k", C.c_int32), ("partitions", C.c_int32), ("k_per_partition", C.c_int32), ("precision", C.c_int32),
        ("device", C.c_int32), ("num_cus", C.c_uint32), ("fixed_width", C.c_uint32), ("multi_q", C.c_uint32), ("multi_pack_us", C.c_uint32), ("multi_bytes", C.c_uint64),
        ("pack_us", C.c_uint32), ("pack_on_device", C.c_uint32), ("claim_sets", C.c_uint32), ("batch_mode", C.c_uint32), ("state_bytes", C.c_uint64),
        ("batch_stream_bytes", C.c_uint64), ("batch_packet_bytes", C.c_uint32), ("batch_compact", C.c_uint32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}


class Cursor(C.Structure):
    """tkspmv_cursor: a position in the result order (search-after paging). row is a GLOBAL row id, score_bits the bit pattern
    of a float32 score; state START ignores both, any state other than START / AFTER acts as END."""
    _fields_ = [("row", C.c_uint32), ("score_bits", C.c_uint32), ("state", C.c_uint32), ("reserved", C.c_uint32)]


class Timing(C.Structure):
    _fields_ = [
        ("stream_kernel_ns", C.c_double), ("select_kernel_ns", C.c_double), ("query_ns", C.c_double),
        ("candidates_avg", C.c_double), ("scores_kernel_ns", C.c_double), ("slow_paths_avg", C.c_double),
        ("appended_avg", C.c_double), ("event_bracket_ns", C.c_double), ("n_queries", C.c_uint32),
        ("reserved", C.c_uint32 * 1),
    ]


class Coo(C.Structure):
    _fields_ = [
        ("rows", C.c_uint32), ("cols", C.c_uint32), ("nnz", C.c_uint64),
        ("row", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_float)),
        ("num_rows_coo", C.c_uint32), ("index_base", C.c_int32), ("symmetric", C.c_int32),
    ]


class OptionsC(C.Structure):
    _fields_ = [
        ("matrix_path", C.c_char * 1024),
        ("use_sample_matrix", C.c_int32), ("reset", C.c_int32), ("num_tests", C.c_int32), ("debug", C.c_int32),
        ("ignore_matrix_values", C.c_int32), ("top_k_value", C.c_int32),
        ("xclbin_path", C.c_char * 1024),
        ("gpu_impl", C.c_int32), ("use_half_precision_gpu", C.c_int32), ("block_size_1d", C.c_int32),
        ("block_size_2d", C.c_int32), ("num_blocks", C.c_int32),
    ]


class FacetBest(C.Structure):
    """tkspmv_facet_best: a bin's best match (facet counts). row is a GLOBAL row id, score_bits the bit pattern of its float32
    score; an empty bin holds (0, 0)."""
    _fields_ = [("row", C.c_uint32), ("score_bits", C.c_uint32)]


class Match(C.Structure):
    """tkspmv_match: a boolean predicate over the 32 clause bits of a row's word W (term predicates): the row matches when
    (W & must) == must, (W & must_not) == 0 and popcount(W & should) >= min_should."""
    _fields_ = [("must", C.c_uint32), ("must_not", C.c_uint32), ("should", C.c_uint32), ("min_should", C.c_uint32)]


# Every symbol include/tkspmv.h declares; tests check the library exports all of them.
EXPORTED_SYMBOLS = [
    "tkspmv_create", "tkspmv_destroy", "tkspmv_get_info", "tkspmv_set_query", "tkspmv_set_query_device",
    "tkspmv_run", "tkspmv_enqueue", "tkspmv_enqueue_many", "tkspmv_enqueue_batch", "tkspmv_enqueue_filtered", "tkspmv_set_filter", "tkspmv_set_groups", "tkspmv_enqueue_grouped", "tkspmv_run_grouped", "tkspmv_enqueue_after", "tkspmv_run_after", "tkspmv_set_boost", "tkspmv_enqueue_boosted", "tkspmv_run_boosted", "tkspmv_enqueue_boosted_range", "tkspmv_run_boosted_range", "tkspmv_enqueue_boosted_facets", "tkspmv_run_boosted_facets", "tkspmv_enqueue_boosted_grouped", "tkspmv_run_boosted_grouped", "tkspmv_enqueue_range", "tkspmv_enqueue_facets", "tkspmv_run_facets", "tkspmv_run_range", "tkspmv_enqueue_match", "tkspmv_run_match", "tkspmv_enqueue_row_vectors", "tkspmv_row_vectors", "tkspmv_run_similar", "tkspmv_enqueue_score_rows", "tkspmv_score_rows", "tkspmv_enqueue_row_stats", "tkspmv_row_stats", "tkspmv_set_boost_cosine", "tkspmv_enqueue_assign", "tkspmv_assign", "tkspmv_enqueue_nearest", "tkspmv_nearest", "tkspmv_enqueue_label_sums", "tkspmv_enqueue_sums_close", "tkspmv_sums_exponent", "tkspmv_label_sums", "tkspmv_enqueue_col_stats", "tkspmv_col_stats", "tkspmv_synchronize", "tkspmv_read", "tkspmv_result_device", "tkspmv_scores", "tkspmv_debug_trace", "tkspmv_debug_counters",
    "tkspmv_time_queries", "tkspmv_time_host_loop", "tkspmv_time_query_batches", "tkspmv_time_stream_read", "tkspmv_enqueue_multi", "tkspmv_time_multi", "tkspmv_profile", "tkspmv_last_error", "tkspmv_device_count", "tkspmv_mtx_read", "tkspmv_mtx_free",
    "tkspmv_mtx_write", "tkspmv_sample_vector", "tkspmv_generate", "tkspmv_generate_rows", "tkspmv_generate_degrees", "tkspmv_options_parse", "tkspmv_pack", "tkspmv_pack_device",
    "tkspmv_sell_roundtrip", "tkspmv_sell_pack_device_check", "tkspmv_packed_info", "tkspmv_packed_decode", "tkspmv_packed_raw", "tkspmv_packed_get_row", "tkspmv_packed_score_rows", "tkspmv_packed_row_stats", "tkspmv_packed_assign", "tkspmv_packed_nearest", "tkspmv_packed_label_sums", "tkspmv_packed_sums_exponent", "tkspmv_sums_close_host", "tkspmv_quantise", "tkspmv_packed_col_stats", "tkspmv_packed_free", "tkspmv_wave_partitions", "tkspmv_packed_save", "tkspmv_packed_load",
    "tkspmv_create_packed",
    "tkspmv_dist_unique_id", "tkspmv_dist_create", "tkspmv_dist_set_batch", "tkspmv_dist_enqueue", "tkspmv_dist_run_many",
    "tkspmv_dist_synchronize", "tkspmv_dist_time_exchange", "tkspmv_dist_read", "tkspmv_dist_destroy", "tkspmv_dist_last_error",
    "tkspmv_merge_topk", "tkspmv_merge_topk_batch", "tkspmv_dist_set_host_exchange", "tkspmv_dist_read_batch",
    "tkspmv_set_option", "tkspmv_get_option", "tkspmv_option_count", "tkspmv_option_info",
]

_lib = None


# int (*)(const void *send, void *recv, uint64_t bytes_per_rank, void *user): the host all-gather of the rehearsal exchange
HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


def lib():
    """Loads libtkspmv.so (once). Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()). "
            "The Top-K SpMV engine has no Python/CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, u32p, f32p, i64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    L.tkspmv_last_error.restype = C.c_char_p
    L.tkspmv_create.argtypes = [C.POINTER(vp), C.POINTER(Desc)]
    L.tkspmv_destroy.argtypes = [vp]
    L.tkspmv_destroy.restype = None
    L.tkspmv_get_info.argtypes = [vp, C.POINTER(Info)]
    L.tkspmv_set_query.argtypes = [vp, f32p, C.POINTER(C.c_double)]
    L.tkspmv_set_query_device.argtypes = [vp, vp]
    L.tkspmv_run.argtypes = [vp, C.POINTER(C.c_double)]
    L.tkspmv_enqueue.argtypes = [vp, vp, vp, vp, vp]
    L.tkspmv_enqueue_many.argtypes = [vp, vp, C.c_int32, C.c_int32, vp]
    L.tkspmv_enqueue_batch.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.tkspmv_enqueue_filtered.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, vp, vp]
    L.tkspmv_set_filter.argtypes = [vp, u32p]
    L.tkspmv_set_groups.argtypes = [vp, u32p, C.c_uint32]
    L.tkspmv_enqueue_grouped.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, vp, vp, vp, vp]
    L.tkspmv_run_grouped.argtypes = [vp, C.c_int32, u32p, f32p, u32p, C.POINTER(C.c_int32)]
    L.tkspmv_enqueue_after.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.tkspmv_run_after.argtypes = [vp, C.POINTER(Cursor), C.c_int32, u32p, f32p, C.POINTER(C.c_int32), u32p, C.POINTER(Cursor)]
    L.tkspmv_set_boost.argtypes = [vp, f32p, f32p]
    L.tkspmv_enqueue_boosted.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.tkspmv_run_boosted.argtypes = [vp, C.POINTER(Cursor), C.c_int32, u32p, f32p, C.POINTER(C.c_int32), u32p, C.POINTER(Cursor)]
    L.tkspmv_enqueue_boosted_range.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, C.c_uint32, vp, vp]
    L.tkspmv_run_boosted_range.argtypes = [vp, C.c_float, C.c_int32, u32p, f32p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.tkspmv_enqueue_boosted_facets.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_uint32, vp, vp, vp, vp]
    L.tkspmv_run_boosted_facets.argtypes = [vp, C.c_float, C.c_int32, u32p, C.POINTER(FacetBest), C.POINTER(C.c_uint64)]
    L.tkspmv_enqueue_boosted_grouped.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp]
    L.tkspmv_run_boosted_grouped.argtypes = [vp, C.c_int32, u32p, f32p, u32p, C.POINTER(C.c_int32)]
    L.tkspmv_enqueue_range.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, C.c_uint32, vp, vp]
    L.tkspmv_run_range.argtypes = [vp, C.c_float, C.c_int32, u32p, f32p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.tkspmv_enqueue_facets.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, vp, C.c_uint32, vp, vp, vp, vp]
    L.tkspmv_run_facets.argtypes = [vp, C.c_float, C.c_int32, u32p, C.POINTER(FacetBest), C.POINTER(C.c_uint64)]
    L.tkspmv_enqueue_match.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, vp]
    L.tkspmv_run_match.argtypes = [vp, u32p, C.POINTER(Match), C.c_int32, C.c_int32, u32p, C.POINTER(C.c_uint64)]
    L.tkspmv_enqueue_row_vectors.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.tkspmv_row_vectors.argtypes = [vp, u32p, C.c_int32, f32p, u32p]
    L.tkspmv_run_similar.argtypes = [vp, u32p, C.c_int32, C.c_int32, u32p, f32p]
    L.tkspmv_enqueue_score_rows.argtypes = [vp, vp, C.c_int32, vp, C.c_int32, C.c_int64, vp, vp]
    L.tkspmv_score_rows.argtypes = [vp, f32p, C.c_int32, u32p, C.c_int32, C.c_int64, f32p]
    L.tkspmv_enqueue_row_stats.argtypes = [vp, C.c_int32, vp, vp]
    L.tkspmv_row_stats.argtypes = [vp, C.c_int32, f32p]
    L.tkspmv_set_boost_cosine.argtypes = [vp]
    L.tkspmv_enqueue_assign.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.tkspmv_assign.argtypes = [vp, f32p, C.c_int32, u32p, f32p]
    L.tkspmv_enqueue_nearest.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.tkspmv_nearest.argtypes = [vp, f32p, C.c_int32, C.c_int32, C.c_int32, u32p, f32p]
    L.tkspmv_enqueue_label_sums.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_uint32, vp, C.c_int32, vp, vp]
    L.tkspmv_enqueue_sums_close.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_int32, vp, vp]
    L.tkspmv_sums_exponent.argtypes = [vp, C.POINTER(C.c_int32)]
    L.tkspmv_label_sums.argtypes = [vp, u32p, C.c_uint32, C.c_int32, C.c_int32, i64p, f32p]
    L.tkspmv_enqueue_col_stats.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp]
    L.tkspmv_col_stats.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.tkspmv_synchronize.argtypes = [vp]
    L.tkspmv_read.argtypes = [vp, u32p, f32p, C.POINTER(C.c_int32)]
    L.tkspmv_result_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.tkspmv_scores.argtypes = [vp, f32p]
    L.tkspmv_debug_trace.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64)]
    L.tkspmv_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int32]
    L.tkspmv_time_queries.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    L.tkspmv_time_host_loop.argtypes = [vp, f32p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tkspmv_time_query_batches.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    L.tkspmv_time_stream_read.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    L.tkspmv_enqueue_multi.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.tkspmv_time_multi.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    L.tkspmv_profile.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(Timing)]
    L.tkspmv_mtx_read.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Coo)]
    L.tkspmv_mtx_free.argtypes = [C.POINTER(Coo)]
    L.tkspmv_mtx_free.restype = None
    L.tkspmv_mtx_write.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u32p, f32p, C.c_int32,
                                   C.c_int32]
    L.tkspmv_sample_vector.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.tkspmv_generate.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint64, C.POINTER(Coo)]
    L.tkspmv_generate_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint64, C.POINTER(Coo)]
    L.tkspmv_generate_degrees.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint64, u32p]
    L.tkspmv_options_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(OptionsC)]
    L.tkspmv_pack.argtypes = [C.POINTER(Desc), C.c_uint32, C.POINTER(vp)]
    L.tkspmv_pack_device.argtypes = [C.POINTER(Desc), C.c_uint32, C.POINTER(vp), C.POINTER(C.c_double)]
    L.tkspmv_packed_info.argtypes = [vp, C.POINTER(Info)]
    L.tkspmv_packed_decode.argtypes = [vp, u32p, u32p, f32p, C.POINTER(C.c_uint64)]
    L.tkspmv_packed_raw.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(u32p), C.POINTER(u32p),
                                    C.POINTER(u32p), C.POINTER(C.c_uint32)]
    L.tkspmv_packed_get_row.argtypes = [vp, C.c_uint32, u32p, f32p, C.c_uint32, u32p]
    L.tkspmv_packed_score_rows.argtypes = [vp, f32p, u32p, C.c_int32, f32p]
    L.tkspmv_packed_row_stats.argtypes = [vp, C.c_int32, f32p]
    L.tkspmv_packed_assign.argtypes = [vp, f32p, C.c_int32, u32p, f32p]
    L.tkspmv_packed_nearest.argtypes = [vp, f32p, C.c_int32, C.c_int32, u32p, u32p, f32p]
    L.tkspmv_packed_label_sums.argtypes = [vp, u32p, C.c_uint32, C.c_int32, C.c_int32, i64p, f32p]
    L.tkspmv_packed_sums_exponent.argtypes = [vp, C.POINTER(C.c_int32)]
    L.tkspmv_sums_close_host.argtypes = [i64p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, f32p]
    L.tkspmv_quantise.argtypes = [C.c_uint32, C.c_int32]
    L.tkspmv_quantise.restype = C.c_int64
    L.tkspmv_packed_col_stats.argtypes = [vp, C.c_int32, u32p, vp]
    L.tkspmv_wave_partitions.argtypes = [C.POINTER(Desc), C.POINTER(C.c_uint32)]
    L.tkspmv_packed_save.argtypes = [vp, C.c_char_p]
    L.tkspmv_packed_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.tkspmv_create_packed.argtypes = [C.POINTER(vp), vp, C.POINTER(Desc)]
    L.tkspmv_packed_free.argtypes = [vp]
    L.tkspmv_packed_free.restype = None
    L.tkspmv_dist_last_error.restype = C.c_char_p
    L.tkspmv_dist_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.tkspmv_dist_create.argtypes = [C.POINTER(vp), vp, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]
    L.tkspmv_dist_set_batch.argtypes = [vp, C.c_int32]
    L.tkspmv_dist_enqueue.argtypes = [vp, vp]
    L.tkspmv_dist_run_many.argtypes = [vp, vp, C.c_int32, C.c_int32]
    L.tkspmv_dist_synchronize.argtypes = [vp]
    L.tkspmv_dist_time_exchange.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    L.tkspmv_dist_read.argtypes = [vp, u32p, f32p, C.POINTER(C.c_int32)]
    L.tkspmv_dist_destroy.argtypes = [vp]
    L.tkspmv_dist_destroy.restype = None
    L.tkspmv_merge_topk.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.tkspmv_merge_topk_batch.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    L.tkspmv_dist_set_host_exchange.argtypes = [vp, HOST_ALLGATHER_FN, vp]
    L.tkspmv_dist_read_batch.argtypes = [vp, u32p, f32p, C.POINTER(C.c_int32)]
    L.tkspmv_set_option.argtypes = [C.c_char_p, C.c_char_p]
    L.tkspmv_get_option.argtypes = [C.c_char_p]
    L.tkspmv_get_option.restype = C.c_char_p
    L.tkspmv_option_info.argtypes = [C.c_int32] + [C.POINTER(C.c_char_p)] * 4
    _lib = L
    return L


def check(status):
    if status != OK:
        raise TkspmvError(status, lib().tkspmv_last_error().decode("utf-8", "replace"))


def ptr(a):
    """A device address or a raw handle (a hipStream_t) as the c_void_p the prototypes take; 0 / None: NULL."""
    return C.c_void_p(int(a)) if a else None


def u32p(arr):
    """A contiguous uint32 numpy array as the typed pointer the prototypes take; None: NULL."""
    return None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_uint32))


def f32p(arr):
    """A contiguous float32 numpy array as the typed pointer the prototypes take; None: NULL."""
    return None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_float))


def i64p(arr):
    """A contiguous int64 numpy array as the typed pointer the prototypes take; None: NULL."""
    return None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int64))


def set_option(name, value):
    """tkspmv_set_option: an engine option (include/tkspmv.h; `options()` lists them) for the engines created after this call.
    value None: back to unset. Raises TkspmvError for a name that is not in the library's table."""
    check(lib().tkspmv_set_option(name.encode(), None if value is None else str(value).encode()))


def get_option(name):
    v = lib().tkspmv_get_option(name.encode())
    return None if v is None else v.decode()


def options():
    """The library's table of options: [{name, kind, values, doc, value}]."""
    L = lib()
    out = []
    for i in range(L.tkspmv_option_count()):
        f = [C.c_char_p() for _ in range(4)]
        check(L.tkspmv_option_info(i, *[C.byref(x) for x in f]))
        name, kind, values, doc = (x.value.decode() for x in f)
        out.append({"name": name, "kind": kind, "values": values, "doc": doc, "value": get_option(name)})
    return out


def check_dist(status):
    if status != OK:
        raise TkspmvError(status, lib().tkspmv_dist_last_error().decode("utf-8", "replace"))
