"""MI355X-native Top-K SpMV engine: host-side mirror of the reference's operator interface for the hot path.

The compute path is hand-written HIP (csrc/engine.hip) behind the C ABI in include/tkspmv.h; this package only
marshals pointers. There is no CPU fallback.
"""
from . import _lib
from ._lib import TkspmvError, set_option, get_option, options, NEAREST_NONE, NEAREST_MAX_N, F32, Q1_7, Q1_7_WIDE, F16, FIXED, Q1_7_F32, MAX_COLS, MAX_K, CURSOR_START, CURSOR_AFTER, CURSOR_END
from .host import CooMatrix, Options, Packed, collapse_topk, page_after, boost_scores, boosted_matches, cosine_weights, inv_l2, nearest, nearest_n, margin, quantise, label_sums, sums_exponent, close_sums, facet_counts, bool_query, match_rows, col_stats, idf_weights, score_bound, create_sample_vector, generate_degrees, generate_matrix, generate_matrix_rows, read_mtx, row_mask, sell_pack_device_check, sell_roundtrip, write_mtx
from .engine import SpMV, topk_spmv, range_spmv, facet_spmv, grouped_spmv, ranked_spmv, boosted_spmv, cosine_spmv, boosted_range_spmv, boosted_facet_spmv, boosted_grouped_spmv, cosine_range_spmv, assign_spmv, nearest_spmv, kmeans_spmv, knn_graph

__all__ = ["SpMV", "topk_spmv", "range_spmv", "facet_spmv", "grouped_spmv", "ranked_spmv", "boosted_spmv", "cosine_spmv", "boosted_range_spmv", "boosted_facet_spmv", "boosted_grouped_spmv", "cosine_range_spmv", "assign_spmv", "nearest_spmv", "kmeans_spmv", "knn_graph", "row_mask", "collapse_topk", "page_after", "boost_scores", "boosted_matches", "cosine_weights", "inv_l2", "nearest", "nearest_n", "margin", "NEAREST_NONE", "NEAREST_MAX_N", "quantise", "label_sums", "sums_exponent", "close_sums", "facet_counts", "bool_query", "match_rows", "col_stats", "idf_weights", "score_bound", "set_option", "get_option", "options", "CooMatrix", "Options", "Packed", "create_sample_vector", "generate_matrix", "generate_matrix_rows", "generate_degrees",
           "read_mtx", "write_mtx", "sell_roundtrip", "sell_pack_device_check", "TkspmvError", "F32", "Q1_7", "Q1_7_WIDE", "F16", "FIXED", "Q1_7_F32", "MAX_COLS", "MAX_K", "CURSOR_START", "CURSOR_AFTER", "CURSOR_END"]


def device_count():
    return _lib.lib().tkspmv_device_count()
