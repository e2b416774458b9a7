// c_api.cpp -- extern "C" surface declared in include/tkspmv.h (plain pointers and sizes only).
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/tkspmv.h"
#include "device_pack.hpp"
#include "engine.hpp"
#include "host_utils.hpp"
#include "options.hpp"
#include "row_lookup.hpp"
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

// The score of one located row from its own packets: reduce_core (kernels/packet_math.hpp) restated lane by lane, what
// score_rows_kernel (kernels/score_rows.hpp) runs on the device. Per packet of the run: products inside the run, +0.0f outside; every
// slot's own ROW_END mask; the carry +0.0f in front of the first packet. Every sum and product is a separately rounded fp32 operation
// (-ffp-contract=off), in the kernel's order. product(value, column word) is the product of one slot inside the run: v * x[col] for a
// score, a function of v alone for a row statistic (row_stats_kernel, kernels/row_stats.hpp).
template <class Product>
static float reduce_located_row(const HostRowView &V, const RowRun &run, Product product) {
    const uint32_t C = V.C;
    float carry = 0.0f, score = 0.0f;
    for (uint32_t pk = run.first_pkt; pk <= run.last_pkt; ++pk) {
        float s[64][8], head[64], tail[64], vv[64], t[64];
        bool end[64][8];
        uint64_t H = 0;  // lanes that hold a row end
        for (uint32_t l = 0; l < 64u; ++l) {
            float p[8];
            for (uint32_t j = 0; j < C; ++j) {
                const uint32_t ss = l * C + j;
                const uint16_t w = V.word(pk, ss);
                const bool inside = (pk > run.first_pkt || ss >= run.first_slot) && (pk < run.last_pkt || ss <= run.last_slot);
                p[j] = inside ? product(V.value(pk, ss), w) : 0.0f;
                end[l][j] = (w & COLW_ROW_END) != 0;
                if (end[l][j]) H |= 1ull << l;
            }
            if (l == 0u) p[0] = p[0] + carry;
            s[l][0] = p[0];
            for (uint32_t j = 1; j < C; ++j) s[l][j] = (end[l][j - 1] ? 0.0f : s[l][j - 1]) + p[j];
            head[l] = s[l][C - 1];
            for (uint32_t j = C - 1; j-- > 0u;)
                if (end[l][j]) head[l] = s[l][j];
            tail[l] = end[l][C - 1] ? 0.0f : s[l][C - 1];
        }
        // the clipped scan: the lane masks of reduce_core, bit for bit
        const uint64_t M1 = ~H, M2 = M1 & (M1 << 1), M4 = M2 & (M2 << 2), M8 = M4 & (M4 << 4);
        const uint64_t X16 = M1 & 0xFFFF0000FFFF0000ull, P16 = X16 & ~(X16 + 0x0001000000010000ull);
        const uint32_t Z32 = (uint32_t)(M1 >> 32);
        const uint64_t P32 = (uint64_t)(Z32 & ~(Z32 + 1u)) << 32;
        for (uint32_t l = 0; l < 64u; ++l) vv[l] = tail[l];
        const uint64_t masks[4] = {M1, M2, M4, M8};
        for (uint32_t step = 0; step < 4u; ++step) {  // row_shr:1, 2, 4, 8 inside each row of 16 lanes; a lane without a source adds +0.0f
            const uint32_t d = 1u << step;
            for (uint32_t l = 0; l < 64u; ++l) t[l] = vv[l] + ((l & 15u) >= d ? vv[l - d] : 0.0f);
            for (uint32_t l = 0; l < 64u; ++l)
                if ((masks[step] >> l) & 1u) vv[l] = t[l];
        }
        for (uint32_t l = 0; l < 64u; ++l) t[l] = ((l >> 4) & 1u) ? vv[(l & ~15u) - 1u] + vv[l] : vv[l];  // row_bcast:15: lane 15 -> row 1, lane 47 -> row 3
        for (uint32_t l = 0; l < 64u; ++l)
            if ((P16 >> l) & 1u) vv[l] = t[l];
        for (uint32_t l = 32; l < 64u; ++l) t[l] = vv[31] + vv[l];  // row_bcast:31: lane 31 -> rows 2 and 3
        for (uint32_t l = 32; l < 64u; ++l)
            if ((P32 >> l) & 1u) vv[l] = t[l];
        carry = vv[63];
        if (pk == run.last_pkt) {  // expand(): the first row end of a lane yields S, later ones their own s[j]
            const uint32_t l = run.last_slot / C, j = run.last_slot % C;
            bool earlier = false;
            for (uint32_t i = 0; i < j; ++i) earlier = earlier || end[l][i];
            const float S = (l == 0u ? 0.0f : vv[l - 1u]) + head[l];
            score = earlier ? s[l][j] : S;
        }
    }
    return score;
}
static float score_located_row(const HostRowView &V, const RowRun &run, const float *x) {
    return reduce_located_row(V, run, [x](float v, uint16_t w) { return v * x[w >> COLW_COL_SHIFT]; });
}
// The cosine weight of a row whose squares sum to l2sq (inv_l2_of, kernels/row_stats.hpp): two separately rounded fp32 operations;
// +0.0f where the sum is 0, +inf or NaN.
static float inv_l2_of(float l2sq) {
    const float w = 1.0f / std::sqrt(l2sq);
    return (l2sq > 0.0f && l2sq < std::numeric_limits<float>::infinity()) ? w : 0.0f;
}

extern "C" {

const char *tkspmv_last_error(void) { return g_err.c_str(); }

int tkspmv_device_count(void) { return device_count(); }

int tkspmv_create(tkspmv_t **out, const tkspmv_desc *desc) {
    if (!out || !desc) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    *out = nullptr;
    std::string err;
    int status = TKSPMV_OK;
    Engine *e = nullptr;
    try {
        e = Engine::create(*desc, err, status);
    } catch (const std::bad_alloc &) {
        return fail(TKSPMV_ERR_NOMEM, "out of host memory while packing");
    }
    if (!e) return fail(status, err);
    *out = new tkspmv_engine{e};
    return TKSPMV_OK;
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

int tkspmv_generate(uint32_t rows, uint32_t cols, uint32_t avg_nnz, int32_t dist, uint64_t seed, tkspmv_coo *out) {
    if (!out || cols == 0 || avg_nnz == 0) return fail(TKSPMV_ERR_INVALID, "bad arguments");
    if (dist != DIST_UNIFORM && dist != DIST_GAMMA) return fail(TKSPMV_ERR_INVALID, "dist must be 0 (uniform) or 1 (gamma)");
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
    if (dist != DIST_UNIFORM && dist != DIST_GAMMA) return fail(TKSPMV_ERR_INVALID, "dist must be 0 (uniform) or 1 (gamma)");
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
    if (dist != DIST_UNIFORM && dist != DIST_GAMMA) return fail(TKSPMV_ERR_INVALID, "dist must be 0 (uniform) or 1 (gamma)");
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

int tkspmv_packed_decode(const tkspmv_packed *p, uint32_t *row, uint32_t *col, float *val, uint64_t *n) {
    if (!p || !n) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    std::vector<uint32_t> r, c;
    std::vector<float> v;
    decode_wbscsr(p->pm, r, c, v);
    *n = r.size();
    if (row) std::memcpy(row, r.data(), r.size() * 4);
    if (col) std::memcpy(col, c.data(), c.size() * 4);
    if (val) std::memcpy(val, v.data(), v.size() * 4);
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
    if (!p || !n || (capacity > 0u && (!col || !val))) return fail(TKSPMV_ERR_INVALID, "NULL argument");
    const PackedMatrix &pm = p->pm;
    if (row >= pm.rows) return fail(TKSPMV_ERR_INVALID, "row out of range (>= rows)");
    if (pm.precision != Precision::F32 && pm.precision != Precision::F32C12)
        return fail(TKSPMV_ERR_UNSUPPORTED, "rows are looked up in fp32 packet streams only (TKSPMV_F32)");
    if (pm.packets.size() != pm.stream_bytes() || pm.pkt_row.size() != pm.n_packets) return fail(TKSPMV_ERR_INVALID, "the packed matrix is incomplete");
    const uint32_t PE = pm.packet_entries;
    const HostRowView V{pm.packets.data(), pm.pkt_row.data(), pm.part_first.data(), pm.part_count.data(), pm.packet_bytes, PE, pm.C,
                        pm.precision == Precision::F32C12};
    RowRun run{0u, 0u, 0u, 0u};
    *n = 0u;
    if (!locate_row(V, row, pm.n_packets, (uint32_t)pm.part_first.size(), PE, run)) return TKSPMV_OK;  // beyond the last stored row
    *n = row_run_entries(run, PE, V.word(run.first_pkt, run.first_slot));
    if (*n == 0u) return TKSPMV_OK;
    uint32_t out = 0u;
    for (uint32_t pk = run.first_pkt; pk <= run.last_pkt && out < capacity; ++pk) {
        const uint32_t s0 = pk == run.first_pkt ? run.first_slot : 0u, s1 = pk == run.last_pkt ? run.last_slot : PE - 1u;
        for (uint32_t ss = s0; ss <= s1 && out < capacity; ++ss, ++out) {
            col[out] = (uint32_t)(V.word(pk, ss) >> COLW_COL_SHIFT);
            val[out] = V.value(pk, ss);
        }
    }
    return TKSPMV_OK;
}

int tkspmv_packed_score_rows(const tkspmv_packed *p, const float *x, const uint32_t *rows, int32_t n_rows, float *scores) {
    if (!p || !x || !rows || !scores || n_rows < 1) return fail(TKSPMV_ERR_INVALID, "bad arguments (packed matrix, vector, rows and scores given, n_rows >= 1)");
    const PackedMatrix &pm = p->pm;
    for (int32_t i = 0; i < n_rows; ++i)
        if (rows[i] >= pm.rows) return fail(TKSPMV_ERR_INVALID, "row out of range (>= rows)");
    if (pm.precision != Precision::F32 && pm.precision != Precision::F32C12)
        return fail(TKSPMV_ERR_UNSUPPORTED, "rows are scored in fp32 packet streams only (TKSPMV_F32)");
    if (pm.packets.size() != pm.stream_bytes() || pm.pkt_row.size() != pm.n_packets) return fail(TKSPMV_ERR_INVALID, "the packed matrix is incomplete");
    const uint32_t PE = pm.packet_entries;
    const HostRowView V{pm.packets.data(), pm.pkt_row.data(), pm.part_first.data(), pm.part_count.data(), pm.packet_bytes, PE, pm.C,
                        pm.precision == Precision::F32C12};
    for (int32_t i = 0; i < n_rows; ++i) {
        RowRun run{0u, 0u, 0u, 0u};
        scores[i] = 0.0f;  // a row without entries: a placeholder, or no packets at all
        if (locate_row(V, rows[i], pm.n_packets, (uint32_t)pm.part_first.size(), PE, run) && row_run_entries(run, PE, V.word(run.first_pkt, run.first_slot)) != 0u)
            scores[i] = score_located_row(V, run, x);
    }
    return TKSPMV_OK;
}

int tkspmv_packed_row_stats(const tkspmv_packed *p, int32_t kind, float *out) {
    if (!p || !out || kind < TKSPMV_ROW_NNZ || kind > TKSPMV_ROW_INV_L2)
        return fail(TKSPMV_ERR_INVALID, "bad arguments (packed matrix and output given, kind = TKSPMV_ROW_NNZ .. TKSPMV_ROW_INV_L2)");
    const PackedMatrix &pm = p->pm;
    if (pm.precision != Precision::F32 && pm.precision != Precision::F32C12)
        return fail(TKSPMV_ERR_UNSUPPORTED, "row statistics are taken from fp32 packet streams only (TKSPMV_F32)");
    if (pm.packets.size() != pm.stream_bytes() || pm.pkt_row.size() != pm.n_packets) return fail(TKSPMV_ERR_INVALID, "the packed matrix is incomplete");
    const uint32_t PE = pm.packet_entries;
    const HostRowView V{pm.packets.data(), pm.pkt_row.data(), pm.part_first.data(), pm.part_count.data(), pm.packet_bytes, PE, pm.C,
                        pm.precision == Precision::F32C12};
    for (uint32_t r = 0; r < pm.rows; ++r) {
        RowRun run{0u, 0u, 0u, 0u};
        out[r] = 0.0f;  // a row without entries: a placeholder, or no packets at all
        if (!locate_row(V, r, pm.n_packets, (uint32_t)pm.part_first.size(), PE, run) || row_run_entries(run, PE, V.word(run.first_pkt, run.first_slot)) == 0u)
            continue;
        switch (kind) {
            case TKSPMV_ROW_NNZ: out[r] = reduce_located_row(V, run, [](float, uint16_t) { return 1.0f; }); break;
            case TKSPMV_ROW_L1: out[r] = reduce_located_row(V, run, [](float v, uint16_t) { return std::fabs(v); }); break;
            case TKSPMV_ROW_L2SQ: out[r] = reduce_located_row(V, run, [](float v, uint16_t) { return v * v; }); break;
            default: out[r] = inv_l2_of(reduce_located_row(V, run, [](float v, uint16_t) { return v * v; })); break;
        }
    }
    return TKSPMV_OK;
}

// col_stats_kernel (kernels/col_stats.hpp) restated as a walk over the stream, from what the device has: the packets, pkt_row and the
// partition table. Per partition: its last row end is looked for from its last packet backwards; the slots up to it, in stream order,
// are its entries -- what lies behind is padding --, a SKIP slot is the placeholder of an empty row, and the row of a slot is the row of
// the partition's first packet plus the row ends in front of it. MAX / MIN compare order keys (order_key, kernels/common.hpp).
int tkspmv_packed_col_stats(const tkspmv_packed *p, int32_t kind, const uint32_t *mask, void *out) {
    if (!p || !out || kind < TKSPMV_COL_NNZ || kind > TKSPMV_COL_MIN)
        return fail(TKSPMV_ERR_INVALID, "bad arguments (packed matrix and output given, kind = TKSPMV_COL_NNZ .. TKSPMV_COL_MIN)");
    const PackedMatrix &pm = p->pm;
    if (pm.precision != Precision::F32 && pm.precision != Precision::F32C12)
        return fail(TKSPMV_ERR_UNSUPPORTED, "column statistics are taken from fp32 packet streams only (TKSPMV_F32)");
    if (pm.packets.size() != pm.stream_bytes() || pm.pkt_row.size() != pm.n_packets) return fail(TKSPMV_ERR_INVALID, "the packed matrix is incomplete");
    const uint32_t PE = pm.packet_entries;
    const HostRowView V{pm.packets.data(), pm.pkt_row.data(), pm.part_first.data(), pm.part_count.data(), pm.packet_bytes, PE, pm.C,
                        pm.precision == Precision::F32C12};
    const auto order_key = [](uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    const uint32_t negate = kind == TKSPMV_COL_MIN ? 0x80000000u : 0u;
    std::vector<uint32_t> acc(pm.cols, 0u);  // counts, or order keys (0: no counted entry)
    for (size_t q = 0; q < pm.part_first.size(); ++q) {
        const uint32_t f0 = pm.part_first[q];
        uint32_t n = 0u, last_slot = 0u;
        for (uint32_t k = pm.part_count[q]; k > 0u; --k)
            if (V.last_end(f0 + k - 1u, last_slot)) {
                n = k;
                break;
            }
        uint32_t r = n ? pm.pkt_row[f0] : 0u;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t lim = k + 1u == n ? last_slot : PE - 1u;
            for (uint32_t ss = 0; ss <= lim; ++ss) {
                const uint16_t w = V.word(f0 + k, ss);
                const uint32_t c = (uint32_t)(w >> COLW_COL_SHIFT);
                const bool allowed = !mask || (r < pm.rows && ((mask[r >> 5] >> (r & 31u)) & 1u));
                if (!(w & COLW_SKIP) && allowed && c < pm.cols) {
                    if (kind == TKSPMV_COL_NNZ) {
                        ++acc[c];
                    } else {
                        uint32_t bits;
                        const float v = V.value(f0 + k, ss);
                        std::memcpy(&bits, &v, 4);
                        acc[c] = std::max(acc[c], order_key(bits ^ negate));
                    }
                }
                if (w & COLW_ROW_END) ++r;
            }
        }
    }
    uint32_t *const o = static_cast<uint32_t *>(out);
    for (uint32_t c = 0; c < pm.cols; ++c) {
        if (kind == TKSPMV_COL_NNZ) {
            o[c] = acc[c];
        } else {  // key_to_float; key 0: -inf; then the negation of MIN undone
            const uint32_t k = acc[c];
            o[c] = (k == 0u ? 0xFF800000u : ((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k)) ^ negate;
        }
    }
    return TKSPMV_OK;
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
    *n = r.size();
    if (row) std::memcpy(row, r.data(), r.size() * 4);
    if (col) std::memcpy(col, c.data(), c.size() * 4);
    if (val) std::memcpy(val, v.data(), v.size() * 4);
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
    const bool fixed_either = desc->precision == TKSPMV_FIXED && (p->pm.precision == Precision::FIXED || p->pm.precision == Precision::FIXED20 || p->pm.precision == Precision::FIXED26);
    const bool f32_either = desc->precision == TKSPMV_F32 && (p->pm.precision == Precision::F32 || p->pm.precision == Precision::F32C12);
    if (!fixed_either && !f32_either && stream_precision(desc->precision) != p->pm.precision)
        d.precision = (p->pm.precision == Precision::F32 || p->pm.precision == Precision::F32C12)
                          ? TKSPMV_F32
                          : (p->pm.precision == Precision::F16
                                 ? TKSPMV_F16
                                 : ((p->pm.precision == Precision::FIXED || p->pm.precision == Precision::FIXED20 || p->pm.precision == Precision::FIXED26)
                                        ? TKSPMV_FIXED
                                        : (p->pm.precision == Precision::Q1_7_RND ? TKSPMV_Q1_7_F32 : TKSPMV_Q1_7)));
    d.fixed_width = (int32_t)p->pm.fixed_width;  // a property of the packed values
    d.nnz_per_lane = (int32_t)p->pm.C;
    std::string err;
    int status = TKSPMV_OK;
    Engine *e = nullptr;
    try {
        e = Engine::create(d, err, status, &p->pm);
    } catch (const std::bad_alloc &) {
        return fail(TKSPMV_ERR_NOMEM, "out of host memory");
    }
    if (!e) return fail(status, err);
    *out = new tkspmv_engine{e};
    return TKSPMV_OK;
}

}  // extern "C"
