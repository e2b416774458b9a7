// c_api.cpp -- extern "C" surface declared in include/tkspmv.h (plain pointers and sizes only).
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/tkspmv.h"
#include "device_pack.hpp"
#include "engine.hpp"
#include "host_utils.hpp"
#include "options.hpp"
#include "packed_host.hpp"
#include "quantise.hpp"
#include "wbscsr.hpp"
#include "wsell.hpp"

using namespace tkspmv;

struct tkspmv_packed {
    PackedMatrix pm;
    int k;
};

static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// Engine::create behind tkspmv_create and tkspmv_create_packed: the handle, or the engine's status and message.
static int create_engine(tkspmv_t **out, const tkspmv_desc &d, const PackedMatrix *prepacked, const char *nomem) {
    std::string err;
    int status = TKSPMV_OK;
    Engine *e = nullptr;
    try {
        e = Engine::create(d, err, status, prepacked);
    } catch (const std::bad_alloc &) {
        return fail(TKSPMV_ERR_NOMEM, nomem);
    }
    if (!e) return fail(status, err);
    *out = new tkspmv_engine{e};
    return TKSPMV_OK;
}

// stream_precision (wbscsr.hpp) backwards: the tkspmv_precision that names a stream's value type. fp32 travels with column words of
// either width, fixed point at any of three widths; truncated Q1.7 has two arithmetic modes and comes back as the narrow one.
static bool is_f32(Precision p) { return p == Precision::F32 || p == Precision::F32C12; }
static bool is_fixed(Precision p) { return p == Precision::FIXED || p == Precision::FIXED20 || p == Precision::FIXED26; }
static int32_t api_precision_of(Precision p) {
    if (is_f32(p)) return TKSPMV_F32;
    if (p == Precision::F16) return TKSPMV_F16;
    if (is_fixed(p)) return TKSPMV_FIXED;
    return p == Precision::Q1_7_RND ? TKSPMV_Q1_7_F32 : TKSPMV_Q1_7;
}

extern "C" {

const char *tkspmv_last_error(void) { return g_err.c_str(); }

int tkspmv_device_count(void) { return device_count(); }

int tkspmv_create(tkspmv_t **out, const tkspmv_desc *desc) {
    if (!out || !desc) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    *out = nullptr;
    return create_engine(out, *desc, nullptr, "out of host memory while packing");
}

void tkspmv_destroy(tkspmv_t *h) {
    if (!h) return;
    delete h->e;
    delete h;
}

#define ENGINE_CALL(call)                                        \
    if (!h) return fail(TKSPMV_ERR_INVALID, "NULL engine");      \
    std::string err;                                             \
    int st = h->e->call;                                         \
    if (st != TKSPMV_OK) g_err = err;                            \
    return st;

// The host twins (packed_host.hpp) behind a packed handle: the argument check with its message, then the twin's status and message.
#define PACKED_CALL(args_ok, bad_args, call)                     \
    if (!(args_ok)) return fail(TKSPMV_ERR_INVALID, bad_args);   \
    std::string err;                                             \
    int st = call;                                               \
    if (st != TKSPMV_OK) g_err = err;                            \
    return st;

int tkspmv_get_info(const tkspmv_t *h, tkspmv_info *info) {
    if (!h || !info) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    h->e->info(info);
    return TKSPMV_OK;
}
int tkspmv_set_query(tkspmv_t *h, const float *host_x, double *elapsed_ns) { ENGINE_CALL(set_query(host_x, elapsed_ns, err)) }
int tkspmv_set_query_device(tkspmv_t *h, const float *dev_x) { ENGINE_CALL(set_query_device(dev_x, err)) }
int tkspmv_run(tkspmv_t *h, double *kernel_ns) { ENGINE_CALL(run(kernel_ns, err)) }
int tkspmv_enqueue(tkspmv_t *h, const float *dev_x, uint32_t *dev_idx, float *dev_val, void *stream) {
    ENGINE_CALL(enqueue(dev_x, dev_idx, dev_val, stream, err))
}
int tkspmv_enqueue_many(tkspmv_t *h, const float *dev_xs, int32_t n_x, int32_t count, void *stream) {
    ENGINE_CALL(enqueue_many(dev_xs, n_x, count, stream, err))
}
int tkspmv_enqueue_batch(tkspmv_t *h, const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream) {
    ENGINE_CALL(enqueue_batch(dev_xs, count, dev_idx, dev_val, stream, err))
}
int tkspmv_enqueue_filtered(tkspmv_t *h, const float *dev_xs, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words,
                            uint32_t *dev_idx, float *dev_val, void *stream) {
    ENGINE_CALL(enqueue_filtered(dev_xs, count, dev_mask, mask_stride_words, dev_idx, dev_val, stream, err))
}
int tkspmv_set_filter(tkspmv_t *h, const uint32_t *host_mask) { ENGINE_CALL(set_filter(host_mask, err)) }
int tkspmv_set_groups(tkspmv_t *h, const uint32_t *host_groups, uint32_t n_groups) { ENGINE_CALL(set_groups(host_groups, n_groups, err)) }
int tkspmv_enqueue_grouped(tkspmv_t *h, const float *dev_xs, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words,
                           uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp, uint32_t *dev_n, void *stream) {
    ENGINE_CALL(enqueue_grouped(dev_xs, count, dev_mask, mask_stride_words, dev_idx, dev_val, dev_grp, dev_n, stream, err))
}
int tkspmv_run_grouped(tkspmv_t *h, int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n) {
    ENGINE_CALL(run_grouped(use_filter, idx, val, grp, n, err))
}
int tkspmv_enqueue_after(tkspmv_t *h, const float *dev_xs, int32_t count, const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask,
                         int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next,
                         void *stream) {
    ENGINE_CALL(enqueue_after(dev_xs, count, dev_cursors, dev_mask, mask_stride_words, dev_idx, dev_val, dev_n, dev_total, dev_next, stream, err))
}
int tkspmv_run_after(tkspmv_t *h, const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total,
                     tkspmv_cursor *next) {
    ENGINE_CALL(run_after(cursor, use_filter, idx, val, n, total, next, err))
}
int tkspmv_set_boost(tkspmv_t *h, const float *host_weight, const float *host_bias) { ENGINE_CALL(set_boost(host_weight, host_bias, err)) }
int tkspmv_enqueue_boosted(tkspmv_t *h, const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                           const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                           uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream) {
    ENGINE_CALL(enqueue_boosted(dev_xs, count, dev_weight, dev_bias, boost_stride, dev_cursors, dev_mask, mask_stride_words, dev_idx, dev_val, dev_n,
                                dev_total, dev_next, stream, err))
}
int tkspmv_run_boosted(tkspmv_t *h, const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total,
                       tkspmv_cursor *next) {
    ENGINE_CALL(run_boosted(cursor, use_filter, idx, val, n, total, next, err))
}
int tkspmv_enqueue_boosted_range(tkspmv_t *h, const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                 const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                                 uint32_t capacity, uint32_t *dev_counts, void *stream) {
    ENGINE_CALL(enqueue_boosted_range(dev_xs, count, dev_weight, dev_bias, boost_stride, dev_thresholds, dev_mask, mask_stride_words, dev_idx, dev_val, capacity,
                                      dev_counts, stream, err))
}
int tkspmv_run_boosted_range(tkspmv_t *h, float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count) {
    ENGINE_CALL(run_boosted_range(threshold, use_filter, idx, val, capacity, count, err))
}
int tkspmv_enqueue_boosted_facets(tkspmv_t *h, const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                  const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words, const uint32_t *dev_labels, uint32_t n_bins,
                                  uint32_t *dev_counts, tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream) {
    ENGINE_CALL(enqueue_boosted_facets(dev_xs, count, dev_weight, dev_bias, boost_stride, dev_thresholds, dev_mask, mask_stride_words, dev_labels, n_bins, dev_counts,
                                       dev_best, dev_totals, stream, err))
}
int tkspmv_run_boosted_facets(tkspmv_t *h, float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total) {
    ENGINE_CALL(run_boosted_facets(threshold, use_filter, counts, best, total, err))
}
int tkspmv_enqueue_boosted_grouped(tkspmv_t *h, const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                   const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp, uint32_t *dev_n,
                                   void *stream) {
    ENGINE_CALL(enqueue_boosted_grouped(dev_xs, count, dev_weight, dev_bias, boost_stride, dev_mask, mask_stride_words, dev_idx, dev_val, dev_grp, dev_n, stream, err))
}
int tkspmv_run_boosted_grouped(tkspmv_t *h, int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n) {
    ENGINE_CALL(run_boosted_grouped(use_filter, idx, val, grp, n, err))
}
int tkspmv_enqueue_range(tkspmv_t *h, const float *dev_xs, int32_t count, const float *dev_thresholds, const uint32_t *dev_mask,
                         int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t capacity, uint32_t *dev_counts, void *stream) {
    ENGINE_CALL(enqueue_range(dev_xs, count, dev_thresholds, dev_mask, mask_stride_words, dev_idx, dev_val, capacity, dev_counts, stream, err))
}
int tkspmv_run_range(tkspmv_t *h, float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count) {
    ENGINE_CALL(run_range(threshold, use_filter, idx, val, capacity, count, err))
}
int tkspmv_enqueue_facets(tkspmv_t *h, const float *dev_xs, int32_t count, const float *dev_thresholds, const uint32_t *dev_mask,
                          int64_t mask_stride_words, const uint32_t *dev_labels, uint32_t n_bins, uint32_t *dev_counts, tkspmv_facet_best *dev_best,
                          uint32_t *dev_totals, void *stream) {
    ENGINE_CALL(enqueue_facets(dev_xs, count, dev_thresholds, dev_mask, mask_stride_words, dev_labels, n_bins, dev_counts, dev_best, dev_totals, stream, err))
}
int tkspmv_run_facets(tkspmv_t *h, float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total) {
    ENGINE_CALL(run_facets(threshold, use_filter, counts, best, total, err))
}
int tkspmv_enqueue_match(tkspmv_t *h, const uint32_t *dev_clauses, int64_t clause_stride_words, const tkspmv_match *dev_preds, int32_t count,
                         const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_out, int64_t out_stride_words, uint32_t *dev_counts, void *stream) {
    ENGINE_CALL(enqueue_match(dev_clauses, clause_stride_words, dev_preds, count, dev_mask, mask_stride_words, dev_out, out_stride_words, dev_counts, stream, err))
}
int tkspmv_run_match(tkspmv_t *h, const uint32_t *host_clauses, const tkspmv_match *pred, int32_t use_filter, int32_t install, uint32_t *host_mask,
                     uint64_t *count) {
    ENGINE_CALL(run_match(host_clauses, pred, use_filter, install, host_mask, count, err))
}
int tkspmv_enqueue_row_vectors(tkspmv_t *h, const uint32_t *dev_rows, int32_t count, float *dev_xs, uint32_t *dev_len, void *stream) {
    ENGINE_CALL(enqueue_row_vectors(dev_rows, count, dev_xs, dev_len, stream, err))
}
int tkspmv_row_vectors(tkspmv_t *h, const uint32_t *host_rows, int32_t count, float *host_xs, uint32_t *host_len) {
    ENGINE_CALL(row_vectors(host_rows, count, host_xs, host_len, err))
}
int tkspmv_run_similar(tkspmv_t *h, const uint32_t *host_rows, int32_t count, int32_t exclude_self, uint32_t *idx, float *val) {
    ENGINE_CALL(run_similar(host_rows, count, exclude_self, idx, val, err))
}
int tkspmv_enqueue_score_rows(tkspmv_t *h, const float *dev_xs, int32_t count, const uint32_t *dev_rows, int32_t n_rows, int64_t rows_stride,
                              float *dev_scores, void *stream) {
    ENGINE_CALL(enqueue_score_rows(dev_xs, count, dev_rows, n_rows, rows_stride, dev_scores, stream, err))
}
int tkspmv_score_rows(tkspmv_t *h, const float *host_xs, int32_t count, const uint32_t *host_rows, int32_t n_rows, int64_t rows_stride,
                      float *host_scores) {
    ENGINE_CALL(score_rows(host_xs, count, host_rows, n_rows, rows_stride, host_scores, err))
}
int tkspmv_enqueue_row_stats(tkspmv_t *h, int32_t kind, float *dev_out, void *stream) { ENGINE_CALL(enqueue_row_stats(kind, dev_out, stream, err)) }
int tkspmv_row_stats(tkspmv_t *h, int32_t kind, float *host_out) { ENGINE_CALL(row_stats(kind, host_out, err)) }
int tkspmv_set_boost_cosine(tkspmv_t *h) { ENGINE_CALL(set_boost_cosine(err)) }
int tkspmv_enqueue_assign(tkspmv_t *h, const float *dev_xs, int32_t count, uint32_t *dev_labels, float *dev_best, void *stream) {
    ENGINE_CALL(enqueue_assign(dev_xs, count, dev_labels, dev_best, stream, err))
}
int tkspmv_assign(tkspmv_t *h, const float *host_xs, int32_t count, uint32_t *host_labels, float *host_best) {
    ENGINE_CALL(assign(host_xs, count, host_labels, host_best, err))
}
int tkspmv_enqueue_label_sums(tkspmv_t *h, const uint32_t *dev_labels, uint32_t n_bins, int32_t quantum_exp, uint32_t flags, int64_t *dev_sums, int32_t mode,
                              float *dev_out, void *stream) {
    ENGINE_CALL(enqueue_label_sums(dev_labels, n_bins, quantum_exp, flags, dev_sums, mode, dev_out, stream, err))
}
int tkspmv_enqueue_sums_close(tkspmv_t *h, const int64_t *dev_sums, uint32_t n_bins, int32_t quantum_exp, int32_t mode, float *dev_out, void *stream) {
    ENGINE_CALL(enqueue_sums_close(dev_sums, n_bins, quantum_exp, mode, dev_out, stream, err))
}
int tkspmv_sums_exponent(tkspmv_t *h, int32_t *quantum_exp) { ENGINE_CALL(sums_exponent(quantum_exp, err)) }
int tkspmv_label_sums(tkspmv_t *h, const uint32_t *host_labels, uint32_t n_bins, int32_t quantum_exp, int32_t mode, int64_t *host_sums, float *host_out) {
    ENGINE_CALL(label_sums(host_labels, n_bins, quantum_exp, mode, host_sums, host_out, err))
}
int tkspmv_enqueue_nearest(tkspmv_t *h, const float *dev_xs, int32_t count, int32_t n, const uint32_t *dev_mask, uint32_t *dev_labels, float *dev_scores, void *stream) {
    ENGINE_CALL(enqueue_nearest(dev_xs, count, n, dev_mask, dev_labels, dev_scores, stream, err))
}
int tkspmv_nearest(tkspmv_t *h, const float *host_xs, int32_t count, int32_t n, int32_t use_filter, uint32_t *host_labels, float *host_scores) {
    ENGINE_CALL(nearest(host_xs, count, n, use_filter, host_labels, host_scores, err))
}
int tkspmv_enqueue_col_stats(tkspmv_t *h, int32_t kind, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, void *dev_out, int64_t out_stride_words,
                             void *stream) {
    ENGINE_CALL(enqueue_col_stats(kind, count, dev_mask, mask_stride_words, dev_out, out_stride_words, stream, err))
}
int tkspmv_col_stats(tkspmv_t *h, int32_t kind, int32_t use_filter, void *host_out) { ENGINE_CALL(col_stats(kind, use_filter, host_out, err)) }
int tkspmv_synchronize(tkspmv_t *h) { ENGINE_CALL(synchronize(err)) }
int tkspmv_read(tkspmv_t *h, uint32_t *idx, float *val, int32_t *n) { ENGINE_CALL(read(idx, val, n, err)) }
int tkspmv_result_device(tkspmv_t *h, const uint32_t **dev_idx, const float **dev_val) {
    if (!h) return fail(TKSPMV_ERR_INVALID, "NULL engine");
    return h->e->result_device(dev_idx, dev_val);
}
int tkspmv_scores(tkspmv_t *h, float *host_y) { ENGINE_CALL(scores(host_y, err)) }
int tkspmv_debug_trace(tkspmv_t *h, uint64_t *host, uint64_t max_words, uint64_t *words) {
    size_t w = 0;
    if (!h) return fail(TKSPMV_ERR_INVALID, "NULL engine");
    std::string err;
    int st = h->e->read_trace(reinterpret_cast<unsigned long long *>(host), (size_t)max_words, &w, err);
    if (st != TKSPMV_OK) g_err = err;
    if (words) *words = w;
    return st;
}
int tkspmv_debug_counters(tkspmv_t *h, uint64_t *out, int32_t n) { ENGINE_CALL(debug_counters(reinterpret_cast<unsigned long long *>(out), n, err)) }
int tkspmv_enqueue_multi(tkspmv_t *h, const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream) {
    ENGINE_CALL(enqueue_multi(dev_xs, count, dev_idx, dev_val, stream, err))
}
int tkspmv_time_multi(tkspmv_t *h, const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query) {
    ENGINE_CALL(time_multi(dev_xs, n_x, iters, ns_per_query, err))
}
int tkspmv_set_option(const char *name, const char *value) {
    if (tkspmv::set_option(name, value) != 0) return fail(TKSPMV_ERR_INVALID, std::string("no such option: ") + (name ? name : "(null)"));
    return TKSPMV_OK;
}
const char *tkspmv_get_option(const char *name) {
    for (int i = 0; i < tkspmv::option_count(); ++i)
        if (name && std::strcmp(tkspmv::option_def(i)->name, name) == 0) return tkspmv::opt(name);
    return nullptr;
}
int tkspmv_option_count(void) { return tkspmv::option_count(); }
int tkspmv_option_info(int32_t i, const char **name, const char **kind, const char **values, const char **doc) {
    const tkspmv::OptionDef *o = tkspmv::option_def(i);
    if (!o) return fail(TKSPMV_ERR_INVALID, "option index out of range");
    if (name) *name = o->name;
    if (kind) *kind = o->kind;
    if (values) *values = o->values;
    if (doc) *doc = o->doc;
    return TKSPMV_OK;
}
int tkspmv_time_query_batches(tkspmv_t *h, const float *dev_xs, int32_t n_x, int32_t iters, int32_t reps, double *ns_per_query) {
    ENGINE_CALL(time_query_batches(dev_xs, n_x, iters, reps, ns_per_query, err))
}
int tkspmv_time_host_loop(tkspmv_t *h, const float *host_xs, int32_t n_x, int32_t iters, double *loop_ns, double *kernel_ns) {
    ENGINE_CALL(time_host_loop(host_xs, n_x, iters, loop_ns, kernel_ns, err))
}
int tkspmv_time_queries(tkspmv_t *h, const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query) {
    ENGINE_CALL(time_queries(dev_xs, n_x, iters, ns_per_query, err))
}
int tkspmv_time_stream_read(tkspmv_t *h, int32_t passes, double *ns_per_pass) {
    ENGINE_CALL(time_stream_read(passes, ns_per_pass, err))
}
int tkspmv_profile(tkspmv_t *h, const float *dev_xs, int32_t n_x, int32_t iters, tkspmv_timing *out) {
    ENGINE_CALL(profile(dev_xs, n_x, iters, out, err))
}

// ---- host helpers ------------------------------------------------------------------------------------
static int coo_to_c(CooMatrix &m, tkspmv_coo *out) {
    std::memset(out, 0, sizeof(*out));
    out->rows = m.rows;
    out->cols = m.cols;
    out->nnz = m.nnz();
    out->num_rows_coo = m.num_rows_coo;
    out->index_base = m.index_base;
    out->symmetric = m.symmetric ? 1 : 0;
    size_t n = m.row.size();
    out->row = (uint32_t *)malloc(std::max<size_t>(n, 1) * 4);
    out->col = (uint32_t *)malloc(std::max<size_t>(n, 1) * 4);
    out->val = (float *)malloc(std::max<size_t>(n, 1) * 4);
    if (!out->row || !out->col || !out->val) {
        free(out->row);
        free(out->col);
        free(out->val);
        std::memset(out, 0, sizeof(*out));
        return fail(TKSPMV_ERR_NOMEM, "out of memory");
    }
    if (n) {
        std::memcpy(out->row, m.row.data(), n * 4);
        std::memcpy(out->col, m.col.data(), n * 4);
        std::memcpy(out->val, m.val.data(), n * 4);
    }
    return TKSPMV_OK;
}

int tkspmv_mtx_read(const char *path, int32_t index_base, int32_t read_values, int32_t sort, tkspmv_coo *out) {
    if (!path || !out) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    CooMatrix m;
    IoError e = read_mtx(path, index_base, read_values != 0, sort != 0, m);
    if (e.code) return fail(e.code, e.message);
    return coo_to_c(m, out);
}

void tkspmv_mtx_free(tkspmv_coo *m) {
    if (!m) return;
    free(m->row);
    free(m->col);
    free(m->val);
    std::memset(m, 0, sizeof(*m));
}

int tkspmv_mtx_write(const char *path, uint32_t rows, uint32_t cols, uint64_t nnz, const uint32_t *row,
                     const uint32_t *col, const float *val, int32_t index_base, int32_t precision) {
    if (!path || (nnz && (!row || !col))) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    IoError e = write_mtx(path, rows, cols, nnz, row, col, val, index_base, precision);
    if (e.code) return fail(e.code, e.message);
    return TKSPMV_OK;
}

int tkspmv_sample_vector(float *vec, int32_t size, int32_t random, int32_t sum_to_one, int32_t norm_one,
                         int32_t seed) {
    if (!vec || size < 0) return fail(TKSPMV_ERR_INVALID, "bad arguments");
    sample_vector(vec, size, random != 0, sum_to_one != 0, norm_one != 0, seed);
    return TKSPMV_OK;
}

static int check_dist(int32_t dist) {
    if (dist != DIST_UNIFORM && dist != DIST_GAMMA) return fail(TKSPMV_ERR_INVALID, "dist must be 0 (uniform) or 1 (gamma)");
    return TKSPMV_OK;
}

int tkspmv_generate(uint32_t rows, uint32_t cols, uint32_t avg_nnz, int32_t dist, uint64_t seed, tkspmv_coo *out) {
    if (!out || cols == 0 || avg_nnz == 0) return fail(TKSPMV_ERR_INVALID, "bad arguments");
    if (const int st = check_dist(dist); st != TKSPMV_OK) return st;
    CooMatrix m;
    try {
        generate_matrix(rows, cols, avg_nnz, dist, seed, m);
    } catch (const std::bad_alloc &) {
        return fail(TKSPMV_ERR_NOMEM, "out of memory");
    }
    return coo_to_c(m, out);
}

int tkspmv_generate_rows(uint32_t row_begin, uint32_t row_end, uint32_t cols, uint32_t avg_nnz, int32_t dist, uint64_t seed,
                         tkspmv_coo *out) {
    if (!out || cols == 0 || avg_nnz == 0 || row_end < row_begin) return fail(TKSPMV_ERR_INVALID, "bad arguments");
    if (const int st = check_dist(dist); st != TKSPMV_OK) return st;
    CooMatrix m;
    try {
        generate_matrix_rows(row_begin, row_end, cols, avg_nnz, dist, seed, m);
    } catch (const std::bad_alloc &) {
        return fail(TKSPMV_ERR_NOMEM, "out of memory");
    }
    return coo_to_c(m, out);
}

int tkspmv_generate_degrees(uint32_t row_begin, uint32_t row_end, uint32_t avg_nnz, int32_t dist, uint64_t seed,
                            uint32_t *deg) {
    if (!deg || avg_nnz == 0 || row_end < row_begin) return fail(TKSPMV_ERR_INVALID, "bad arguments");
    if (const int st = check_dist(dist); st != TKSPMV_OK) return st;
    generate_degrees(row_begin, row_end, avg_nnz, dist, seed, deg);
    return TKSPMV_OK;
}

int tkspmv_options_parse(int argc, char **argv, tkspmv_options *out) {
    if (!out || (argc > 0 && !argv)) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    Options o(argc, argv);
    std::memset(out, 0, sizeof(*out));
    std::strncpy(out->matrix_path, o.matrix_path.c_str(), sizeof(out->matrix_path) - 1);
    std::strncpy(out->xclbin_path, o.xclbin_path.c_str(), sizeof(out->xclbin_path) - 1);
    out->use_sample_matrix = o.use_sample_matrix;
    out->reset = o.reset;
    out->num_tests = (int32_t)o.num_tests;
    out->debug = o.debug;
    out->ignore_matrix_values = o.ignore_matrix_values;
    out->top_k_value = o.top_k_value;
    out->gpu_impl = o.gpu_impl;
    out->use_half_precision_gpu = o.use_half_precision_gpu;
    out->block_size_1d = o.block_size_1d;
    out->block_size_2d = o.block_size_2d;
    out->num_blocks = o.num_blocks;
    return TKSPMV_OK;
}

int tkspmv_pack(const tkspmv_desc *d, uint32_t n_wave_partitions_hint, tkspmv_packed **out) {
    if (!d || !out) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    *out = nullptr;
    tkspmv_packed *p = new tkspmv_packed();
    int kind = 0;
    uint32_t C = entries_per_lane_of(*d);
    const Precision sp = stream_precision_of(*d);
    std::string err = pack_wbscsr(d->rows, d->cols, d->nnz, d->row, d->col, d->val, sp, C,
                                  n_wave_partitions_hint ? n_wave_partitions_hint : 4096u, min_packets_per_partition_for(d->nnz, C, d->cols), p->pm, kind,
                                  fixed_width_of(*d));
    if (!err.empty()) {
        delete p;
        return fail(kind == 2 ? TKSPMV_ERR_NOT_SORTED : TKSPMV_ERR_INVALID, err);
    }
    p->k = d->k;
    *out = p;
    return TKSPMV_OK;
}

int tkspmv_pack_device(const tkspmv_desc *d, uint32_t n_wave_partitions_hint, tkspmv_packed **out, double *ms) {
    if (!d || !out) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (device_count() < 1) return fail(TKSPMV_ERR_DEVICE, "no HIP device available (the device packer needs one)");
    std::string serr;
    if (use_device(d->device, serr) != TKSPMV_OK) return fail(TKSPMV_ERR_DEVICE, serr);
    DevicePacked dp;
    int kind = 0;
    std::string err = pack_wbscsr_device(d->rows, d->cols, d->nnz, d->row, d->col, d->val, stream_precision_of(*d),
                                         entries_per_lane_of(*d), n_wave_partitions_hint ? n_wave_partitions_hint : 4096u,
                                         min_packets_per_partition_for(d->nnz, entries_per_lane_of(*d), d->cols),
                                         fixed_width_of(*d), dp, kind);
    if (err.empty()) err = download_device_packed(dp);
    free_device_packed(dp);
    if (!err.empty()) return fail(kind == 2 ? TKSPMV_ERR_NOT_SORTED : (err.find("failed:") != std::string::npos ? TKSPMV_ERR_DEVICE : TKSPMV_ERR_INVALID), err);
    tkspmv_packed *p = new tkspmv_packed();
    p->pm = std::move(dp.meta);
    p->k = d->k;
    if (ms) {
        ms[0] = dp.upload_ms;
        ms[1] = dp.kernels_ms;
    }
    *out = p;
    return TKSPMV_OK;
}

int tkspmv_packed_info(const tkspmv_packed *p, tkspmv_info *info) {
    if (!p || !info) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    fill_info(p->pm, p->k, info);
    return TKSPMV_OK;
}

// A decoded matrix into the caller's arrays (each optional) and its number of entries into *n.
static void copy_out_coo(const std::vector<uint32_t> &r, const std::vector<uint32_t> &c, const std::vector<float> &v, uint32_t *row, uint32_t *col,
                         float *val, uint64_t *n) {
    *n = r.size();
    if (row) std::memcpy(row, r.data(), r.size() * 4);
    if (col) std::memcpy(col, c.data(), c.size() * 4);
    if (val) std::memcpy(val, v.data(), v.size() * 4);
}

int tkspmv_packed_decode(const tkspmv_packed *p, uint32_t *row, uint32_t *col, float *val, uint64_t *n) {
    if (!p || !n) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    std::vector<uint32_t> r, c;
    std::vector<float> v;
    decode_wbscsr(p->pm, r, c, v);
    copy_out_coo(r, c, v, row, col, val, n);
    return TKSPMV_OK;
}

int tkspmv_packed_raw(const tkspmv_packed *p, const void **packets, uint64_t *packet_bytes, const uint32_t **pkt_row,
                      const uint32_t **part_first, const uint32_t **part_count, uint32_t *n_parts) {
    if (!p) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    if (packets) *packets = p->pm.packets.data();
    if (packet_bytes) *packet_bytes = p->pm.packet_bytes;
    if (pkt_row) *pkt_row = p->pm.pkt_row.data();
    if (part_first) *part_first = p->pm.part_first.data();
    if (part_count) *part_count = p->pm.part_count.data();
    if (n_parts) *n_parts = (uint32_t)p->pm.part_first.size();
    return TKSPMV_OK;
}

int tkspmv_packed_get_row(const tkspmv_packed *p, uint32_t row, uint32_t *col, float *val, uint32_t capacity, uint32_t *n) {
    PACKED_CALL(p && n && (capacity == 0u || (col && val)), "NULL argument", packed_get_row(p->pm, row, col, val, capacity, n, err))
}
int tkspmv_packed_score_rows(const tkspmv_packed *p, const float *x, const uint32_t *rows, int32_t n_rows, float *scores) {
    PACKED_CALL(p && x && rows && scores && n_rows >= 1, "bad arguments (packed matrix, vector, rows and scores given, n_rows >= 1)",
                packed_score_rows(p->pm, x, rows, n_rows, scores, err))
}
int tkspmv_packed_row_stats(const tkspmv_packed *p, int32_t kind, float *out) {
    PACKED_CALL(p && out && kind >= TKSPMV_ROW_NNZ && kind <= TKSPMV_ROW_INV_L2,
                "bad arguments (packed matrix and output given, kind = TKSPMV_ROW_NNZ .. TKSPMV_ROW_INV_L2)", packed_row_stats(p->pm, kind, out, err))
}
int tkspmv_packed_assign(const tkspmv_packed *p, const float *xs, int32_t count, uint32_t *labels, float *best) {
    PACKED_CALL(p && xs && labels && count >= 1, "bad arguments (packed matrix, vectors and labels given, count >= 1)", packed_assign(p->pm, xs, count, labels, best, err))
}
int tkspmv_packed_nearest(const tkspmv_packed *p, const float *xs, int32_t count, int32_t n, const uint32_t *mask, uint32_t *labels, float *scores) {
    PACKED_CALL(p && xs && labels && scores && count >= 1 && n >= 1 && n <= TKSPMV_NEAREST_MAX_N,
                "bad arguments (packed matrix, vectors, labels and scores given, count >= 1, n = 1 .. TKSPMV_NEAREST_MAX_N)",
                packed_nearest(p->pm, xs, count, n, mask, labels, scores, err))
}
int tkspmv_packed_label_sums(const tkspmv_packed *p, const uint32_t *labels, uint32_t n_bins, int32_t quantum_exp, int32_t mode, int64_t *sums, float *out) {
    PACKED_CALL(p && labels && n_bins >= 1u && n_bins <= (1u << 30) && mode >= TKSPMV_SUMS_RAW && mode <= TKSPMV_SUMS_UNIT && (mode == TKSPMV_SUMS_RAW || out),
                "bad arguments (packed matrix and labels given, 1 <= n_bins <= 2^30, mode = TKSPMV_SUMS_RAW .. TKSPMV_SUMS_UNIT, out given unless RAW)",
                packed_label_sums(p->pm, labels, n_bins, quantum_exp, mode, sums, out, err))
}
int tkspmv_packed_sums_exponent(const tkspmv_packed *p, int32_t *quantum_exp) {
    PACKED_CALL(p && quantum_exp, "bad arguments (packed matrix and output given)", packed_sums_exponent(p->pm, quantum_exp, err))
}
int tkspmv_sums_close_host(const int64_t *sums, uint32_t n_bins, uint32_t cols, int32_t quantum_exp, int32_t mode, float *out) {
    if (!sums || !out || (mode != TKSPMV_SUMS_FLOAT && mode != TKSPMV_SUMS_UNIT)) return fail(TKSPMV_ERR_INVALID, "bad arguments (sums and out given, mode = TKSPMV_SUMS_FLOAT or TKSPMV_SUMS_UNIT)");
    sums_close_host(sums, n_bins, cols, quantum_exp, mode, out);
    return TKSPMV_OK;
}
int64_t tkspmv_quantise(uint32_t value_bits, int32_t quantum_exp) { return quantise(value_bits, quantum_exp); }
int tkspmv_packed_col_stats(const tkspmv_packed *p, int32_t kind, const uint32_t *mask, void *out) {
    PACKED_CALL(p && out && kind >= TKSPMV_COL_NNZ && kind <= TKSPMV_COL_MIN,
                "bad arguments (packed matrix and output given, kind = TKSPMV_COL_NNZ .. TKSPMV_COL_MIN)", packed_col_stats(p->pm, kind, mask, out, err))
}

void tkspmv_packed_free(tkspmv_packed *p) { delete p; }

int tkspmv_sell_roundtrip(const tkspmv_desc *d, uint32_t n_wave_partitions_hint, uint32_t *row, uint32_t *col, float *val,
                          uint64_t *n, uint64_t *info) {
    if (!d || !n) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    SellMatrix sm;
    const std::string err = pack_wsell(d->rows, d->cols, d->nnz, d->row, d->col, d->val,
                                       n_wave_partitions_hint ? n_wave_partitions_hint : 4088u, sm,
                                       d->precision == TKSPMV_Q1_7_F32 ? SellValues::Q1_7_RND : SellValues::F32);
    if (!err.empty()) return fail(TKSPMV_ERR_INVALID, err);
    std::vector<uint32_t> r, c;
    std::vector<float> v;
    decode_wsell(sm, r, c, v);
    copy_out_coo(r, c, v, row, col, val, n);
    if (info) {
        uint32_t most = 0;
        for (uint32_t pc : sm.part_count) most = std::max(most, pc);
        info[0] = sm.n_slices;
        info[1] = sm.n_chunks;
        info[2] = sm.padded_entries;
        info[3] = sm.part_first.size();
        info[4] = sm.stream_bytes();
        info[5] = most;
    }
    return TKSPMV_OK;
}

int tkspmv_sell_pack_device_check(const tkspmv_desc *d, uint32_t n_wave_partitions_hint, uint64_t *info, double *ms) {
    if (!d || !info) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    if (device_count() < 1) return fail(TKSPMV_ERR_DEVICE, "no HIP device available (the device packer needs one)");
    std::string serr;
    if (use_device(d->device, serr) != TKSPMV_OK) return fail(TKSPMV_ERR_DEVICE, serr);
    const uint32_t hint = n_wave_partitions_hint ? n_wave_partitions_hint : 4088u;
    const SellValues sv = d->precision == TKSPMV_Q1_7_F32 ? SellValues::Q1_7_RND : SellValues::F32;
    SellMatrix host;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string herr = pack_wsell(d->rows, d->cols, d->nnz, d->row, d->col, d->val, hint, host, sv);
    const auto t1 = std::chrono::steady_clock::now();
    DeviceSell ds;
    std::string derr = pack_wsell_device(d->rows, d->cols, d->nnz, d->row, d->col, d->val, hint, sv, nullptr, nullptr, ds);
    if (herr != derr) {
        free_device_sell(ds);
        return fail(TKSPMV_ERR_STATE, "the two packers disagree on the input: host '" + herr + "', device '" + derr + "'");
    }
    if (!herr.empty()) return fail(TKSPMV_ERR_INVALID, herr);
    derr = download_device_sell(ds);
    free_device_sell(ds);
    if (!derr.empty()) return fail(TKSPMV_ERR_DEVICE, derr);
    const SellMatrix &dev = ds.meta;
    info[0] = (host.n_slices == dev.n_slices && host.n_chunks == dev.n_chunks && host.packet_bytes == dev.packet_bytes &&
               host.padded_entries == dev.padded_entries && host.packets == dev.packets && host.slice_rows == dev.slice_rows &&
               host.part_first == dev.part_first && host.part_count == dev.part_count && host.part_slice0 == dev.part_slice0)
                  ? 1u : 0u;
    info[1] = host.stream_bytes();
    info[2] = host.n_chunks;
    if (ms) {
        ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        ms[1] = ds.plan_ms;
        ms[2] = ds.upload_ms;
        ms[3] = ds.kernels_ms;
    }
    return TKSPMV_OK;
}

int tkspmv_packed_save(const tkspmv_packed *p, const char *path) {
    if (!p || !path) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    const std::string err = save_packed(p->pm, path);
    if (!err.empty()) return fail(TKSPMV_ERR_IO, err);
    return TKSPMV_OK;
}

int tkspmv_packed_load(const char *path, tkspmv_packed **out) {
    if (!path || !out) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    *out = nullptr;
    tkspmv_packed *p = new tkspmv_packed();
    const std::string err = load_packed(path, p->pm);
    if (!err.empty()) {
        delete p;
        return fail(TKSPMV_ERR_IO, err);
    }
    p->k = 0;
    *out = p;
    return TKSPMV_OK;
}

int tkspmv_wave_partitions(const tkspmv_desc *desc, uint32_t *n) {
    if (!desc || !n) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    std::string err;
    int st = wave_partitions_for(*desc, n, err);
    if (st != TKSPMV_OK) g_err = err;
    return st;
}

int tkspmv_create_packed(tkspmv_t **out, const tkspmv_packed *p, const tkspmv_desc *desc) {
    if (!out || !p || !desc) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    *out = nullptr;
    tkspmv_desc d = *desc;
    d.rows = p->pm.rows;
    d.cols = p->pm.cols;
    d.nnz = p->pm.nnz;
    // desc.precision chooses among the arithmetic modes of the packed value type (only Q1.7 has two)
    const bool fixed_either = desc->precision == TKSPMV_FIXED && is_fixed(p->pm.precision);
    const bool f32_either = desc->precision == TKSPMV_F32 && is_f32(p->pm.precision);
    if (!fixed_either && !f32_either && stream_precision(desc->precision) != p->pm.precision) d.precision = api_precision_of(p->pm.precision);
    d.fixed_width = (int32_t)p->pm.fixed_width;  // a property of the packed values
    d.nnz_per_lane = (int32_t)p->pm.C;
    return create_engine(out, d, &p->pm, "out of host memory");
}

}  // extern "C"
