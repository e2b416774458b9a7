// engine.hpp -- device engine behind the C ABI (include/tkspmv.h). Mirrors the reference's per-back-end
// `struct SpMV` (host_spmv_bscsr.cpp:79-485, host_spmv_topk_csr_gpu.cu:44-263): setup once, then per
// query reset(vec) -> operator()() -> read_result().
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/tkspmv.h"
#include "wbscsr.hpp"

namespace tkspmv {

struct EngineImpl;  // HIP state lives in engine.hip

class Engine {
   public:
    // Returns nullptr and fills err/status on failure.
    // prepacked: a matrix packed earlier (then desc.row/col/val are not read)
    static Engine *create(const tkspmv_desc &desc, std::string &err, int &status, const PackedMatrix *prepacked = nullptr);
    ~Engine();

    int set_query(const float *host_x, double *elapsed_ns, std::string &err);
    int set_query_device(const float *dev_x, std::string &err);
    int run(double *kernel_ns, std::string &err);
    int enqueue(const float *dev_x, uint32_t *dev_idx, float *dev_val, void *stream, std::string &err);
    int enqueue_many(const float *dev_xs, int32_t n_x, int32_t count, void *stream, std::string &err);
    int enqueue_batch(const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream,
                      std::string &err);
    // Queries in passes of several per matrix pass (multi_kernel); same contract as enqueue_batch.
    int enqueue_multi(const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream, std::string &err);
    int time_multi(const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query, std::string &err);
    // Filtered top-k (stream_filter_kernel): query i restricted to the rows set in dev_mask + i * mask_stride_words.
    int enqueue_filtered(const float *dev_xs, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx,
                         float *dev_val, void *stream, std::string &err);
    int set_filter(const uint32_t *host_mask, std::string &err);
    // Grouped top-k (group_best_kernel): every row carries a label (set_groups; NULL removes them); a query returns the k best groups,
    // each by its best eligible row, with that row's group id. run_grouped is the host-side counterpart (installed vector, waits).
    int set_groups(const uint32_t *host_groups, uint32_t n_groups, std::string &err);
    int enqueue_grouped(const float *dev_xs, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                        uint32_t *dev_grp, uint32_t *dev_n, void *stream, std::string &err);
    int run_grouped(int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n, std::string &err);
    // Search-after paging (after_cut_kernel): the k eligible rows that rank strictly behind a cursor, with the hits left and the cursor
    // of the following page. run_after is the host-side counterpart (installed vector, host cursor, waits).
    int enqueue_after(const float *dev_xs, int32_t count, const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words,
                      uint32_t *dev_idx, float *dev_val, uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream, std::string &err);
    int run_after(const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total, tkspmv_cursor *next,
                  std::string &err);
    // Boosted top-k (boost_cut_kernel): search-after pages over s' = weight[r] * s + bias[r] (two separately rounded fp32 operations;
    // either array may be absent), on the search-after path's scratch. set_boost installs the pair that both-NULL calls and run_boosted,
    // the host-side counterpart of run_after, name; both NULL removes it.
    int set_boost(const float *host_weight, const float *host_bias, std::string &err);
    int enqueue_boosted(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                        const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                        uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream, std::string &err);
    int run_boosted(const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total, tkspmv_cursor *next,
                    std::string &err);
    // Boosted range, facet and grouped queries (boosted_hits_kernel, boosted_bins_kernel; boost_cut_kernel in front of the grouped path):
    // enqueue_range's, enqueue_facets' and enqueue_grouped's contracts read on enqueue_boosted's s', with its weight / bias / stride
    // behind `count`. The first two run on the search-after path's scratch, the third on the grouped path's. The run_* forms are the
    // host-side counterparts (installed vector, boost, mask and labels; wait).
    int enqueue_boosted_range(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                              const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                              uint32_t capacity, uint32_t *dev_counts, void *stream, std::string &err);
    int run_boosted_range(float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count, std::string &err);
    int enqueue_boosted_facets(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                               const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words, const uint32_t *dev_labels, uint32_t n_bins,
                               uint32_t *dev_counts, tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream, std::string &err);
    int run_boosted_facets(float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total, std::string &err);
    int enqueue_boosted_grouped(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp, uint32_t *dev_n,
                                void *stream, std::string &err);
    int run_boosted_grouped(int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n, std::string &err);
    // Range queries (range_kernel): every allowed row with entries that scores >= the query's threshold, unordered; run_range is
    // the host-side counterpart (installed vector, host threshold, waits, sorts).
    int enqueue_range(const float *dev_xs, int32_t count, const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words,
                      uint32_t *dev_idx, float *dev_val, uint32_t capacity, uint32_t *dev_counts, void *stream, std::string &err);
    int run_range(float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count, std::string &err);
    // Facet counts (facet_kernel): a range query's matches per label -- how many, and which comes first in the result order --
    // instead of the matches themselves; run_facets is the host-side counterpart (installed vector and labels, host threshold, waits).
    int enqueue_facets(const float *dev_xs, int32_t count, const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words,
                       const uint32_t *dev_labels, uint32_t n_bins, uint32_t *dev_counts, tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream,
                       std::string &err);
    int run_facets(float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total, std::string &err);
    // Term predicates (match_kernel): the allow-mask of the rows whose own columns satisfy a boolean predicate over up to 32 clauses
    // (sets of columns), made on the device from the packets' column plane; run_match is the host-side counterpart (host table and
    // predicate, waits, optionally installs the result as the engine's filter).
    int enqueue_match(const uint32_t *dev_clauses, int64_t clause_stride_words, const tkspmv_match *dev_preds, int32_t count, const uint32_t *dev_mask,
                      int64_t mask_stride_words, uint32_t *dev_out, int64_t out_stride_words, uint32_t *dev_counts, void *stream, std::string &err);
    int run_match(const uint32_t *host_clauses, const tkspmv_match *pred, int32_t use_filter, int32_t install, uint32_t *host_mask, uint64_t *count,
                  std::string &err);
    // Queries by stored row (row_vectors_kernel): rows of the matrix, given by the global ids queries return, expanded into the dense
    // vectors every enqueue_* call takes; run_similar = the engine's top-k with each given row as the query (chunks on engine-owned
    // scratch: ids up, row vectors, the batch sequence, wait, results down), the row itself removed from its list on request.
    int enqueue_row_vectors(const uint32_t *dev_rows, int32_t count, float *dev_xs, uint32_t *dev_len, void *stream, std::string &err);
    int row_vectors(const uint32_t *host_rows, int32_t count, float *host_xs, uint32_t *host_len, std::string &err);
    int run_similar(const uint32_t *host_rows, int32_t count, int32_t exclude_self, uint32_t *idx, float *val, std::string &err);
    // Scores of given rows (score_rows_kernel): what the rows dev_rows + q * rows_stride [0 .. n_rows) (global ids) score for query q, from
    // the rows' own packets -- no pass over the matrix; score_rows is the host-side counterpart (chunks on engine-owned scratch, waits).
    int enqueue_score_rows(const float *dev_xs, int32_t count, const uint32_t *dev_rows, int32_t n_rows, int64_t rows_stride, float *dev_scores,
                           void *stream, std::string &err);
    int score_rows(const float *host_xs, int32_t count, const uint32_t *host_rows, int32_t n_rows, int64_t rows_stride, float *host_scores,
                   std::string &err);
    // Row statistics (row_stats_kernel): one float per local row -- entry count, L1 norm, squared L2 norm or the cosine weight 1 / L2 --
    // from one pass over the packet stream, summed in the streaming kernels' order; row_stats is the host-side counterpart (engine-owned
    // scratch, waits); set_boost_cosine installs the cosine weights as the boost (set_boost(w, NULL)'s state) without leaving the device.
    int enqueue_row_stats(int32_t kind, float *dev_out, void *stream, std::string &err);
    int row_stats(int32_t kind, float *host_out, std::string &err);
    int set_boost_cosine(std::string &err);
    // Assignment (assign_kernel): for every local row the index of the best-scoring of `count` vectors (ties: the smallest) and that
    // score, the bits every scoring path reports; one pass over the packet stream per 16384 / column tier vectors. dev_best = NULL:
    // one pass only. assign is the host-side counterpart (engine-owned scratch, chunks of vectors, waits for its own launches).
    int enqueue_assign(const float *dev_xs, int32_t count, uint32_t *dev_labels, float *dev_best, void *stream, std::string &err);
    int assign(const float *host_xs, int32_t count, uint32_t *host_labels, float *host_best, std::string &err);
    // Nearest-n assignment (nearest_fill_kernel, nearest_kernel): for every local row its n best-scoring of `count` vectors in order
    // (score descending, ties by index ascending), labels[rows][n] and scores[rows][n]; dev_mask, if given, restricts the rows
    // (one bit per local row; the others get TKSPMV_NEAREST_NONE and -inf throughout). nearest is the host-side counterpart
    // (engine-owned scratch, chunks of vectors, waits for its own launches; use_filter: among the rows of the installed mask).
    int enqueue_nearest(const float *dev_xs, int32_t count, int32_t n, const uint32_t *dev_mask, uint32_t *dev_labels, float *dev_scores, void *stream, std::string &err);
    int nearest(const float *host_xs, int32_t count, int32_t n, int32_t use_filter, uint32_t *host_labels, float *host_scores, std::string &err);
    // Label sums (label_sums_kernel): per label the column sums of the local rows, as int64 multiples of 2^quantum_exp (quantise.hpp),
    // exact and bit-identical whatever the geometry or the order of the atomics; mode FLOAT / UNIT adds the closing launch
    // (label_sums_close_kernel), which enqueue_sums_close runs alone, e.g. over merged shard sums. sums_exponent is the default
    // exponent, from three col_stats passes (waits); label_sums is the host-side counterpart (engine-owned scratch, waits).
    int enqueue_label_sums(const uint32_t *dev_labels, uint32_t n_bins, int32_t quantum_exp, uint32_t flags, int64_t *dev_sums, int32_t mode, float *dev_out,
                           void *stream, std::string &err);
    int enqueue_sums_close(const int64_t *dev_sums, uint32_t n_bins, int32_t quantum_exp, int32_t mode, float *dev_out, void *stream, std::string &err);
    int sums_exponent(int32_t *quantum_exp, std::string &err);
    int label_sums(const uint32_t *host_labels, uint32_t n_bins, int32_t quantum_exp, int32_t mode, int64_t *host_sums, float *host_out, std::string &err);
    // Column statistics (col_stats_kernel): one word per column and set of rows -- the number of stored entries (uint32) or the largest /
    // smallest stored value (float32) --, a set being all rows or the rows of an allow-mask; exact whatever the order of the atomics.
    // col_stats is the host-side counterpart (engine-owned scratch, waits; use_filter: among the rows of the installed mask).
    int enqueue_col_stats(int32_t kind, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, void *dev_out, int64_t out_stride_words,
                          void *stream, std::string &err);
    int col_stats(int32_t kind, int32_t use_filter, void *host_out, std::string &err);
    // enqueue_list through the multi-query path when the engine has one (desc.multi_q), else the ordinary sequence
    int enqueue_multi_list(const float *const *dev_xs, uint32_t *const *dev_idx, float *const *dev_val, int32_t count,
                           void *stream, std::string &err);
    // A back-to-back sequence given as lists of device pointers (count entries each); complete in stream order.
    int enqueue_list(const float *const *dev_xs, uint32_t *const *dev_idx, float *const *dev_val, int32_t count,
                     void *stream, std::string &err);
    // Deferred selection (back-to-back sequences on ONE stream): the top-k of a query is selected inside the next
    // enqueue_deferred launch, or by drain(). Results are complete in stream order only after drain().
    int enqueue_deferred(const float *dev_x, uint32_t *dev_idx, float *dev_val, void *stream, std::string &err);
    int drain(void *stream, std::string &err);
    int synchronize(std::string &err);
    int read(uint32_t *idx, float *val, int32_t *n, std::string &err);
    int result_device(const uint32_t **dev_idx, const float **dev_val);
    int scores(float *host_y, std::string &err);
    int read_trace(unsigned long long *host, size_t max_words, size_t *words, std::string &err);
    int debug_counters(unsigned long long *out, int n, std::string &err);
    int time_queries(const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query, std::string &err);
    int time_host_loop(const float *host_xs, int32_t n_x, int32_t iters, double *loop_ns, double *kernel_ns, std::string &err);
    int time_query_batches(const float *dev_xs, int32_t n_x, int32_t iters, int32_t reps, double *ns_per_query, std::string &err);
    int time_stream_read(int32_t passes, double *ns_per_pass, std::string &err);
    int profile(const float *dev_xs, int32_t n_x, int32_t iters, tkspmv_timing *out, std::string &err);
    void info(tkspmv_info *out) const;

   private:
    Engine() = default;
    EngineImpl *impl_ = nullptr;
};

void fill_info(const PackedMatrix &pm, int k, tkspmv_info *out);
uint64_t algorithmic_bytes(uint64_t nnz, uint32_t rows, uint32_t cols, uint32_t value_bytes, int k);
int device_count();
int use_device(int device, std::string &err);  // hipSetDevice(device), or the current device for -1
// Entries per lane and packet: desc.nnz_per_lane, by default 4. (8, where those kernels exist -- fp32 values, at most
// 1024 columns -- is opt-in: 3-4 % faster on the BASELINE matrix in short probes, 10-15 % slower in bench.py's
// conditions (64 query vectors, 4 stream copies), 3x slower at 2-3M rows, where its longer partitions overflow the
// private candidate lists.)
inline uint32_t entries_per_lane_of(const tkspmv_desc &d) {
    return d.nnz_per_lane > 0 ? (uint32_t)d.nnz_per_lane : 4u;
}
// Bits per value of a descriptor: desc.fixed_width for TKSPMV_FIXED (0 => 32, the reference's default FIXED_WIDTH), 0 for
// every other precision (where a non-zero fixed_width is rejected by the packer).
inline uint32_t fixed_width_of(const tkspmv_desc &d) {
    if (d.precision != TKSPMV_FIXED) return (uint32_t)d.fixed_width;
    return d.fixed_width == 0 ? 32u : (uint32_t)d.fixed_width;
}
// Value type of the packet stream a descriptor asks for (at most 1024 columns: narrow fixed point travels bit-packed, FIXED20,
// and fp32 values with 12-bit column words, F32C12).
inline Precision stream_precision_of(const tkspmv_desc &d) {
    return stream_precision(d.precision, fixed_width_of(d), d.cols, entries_per_lane_of(d));
}
// Wave partitions tkspmv_create would cut the matrix into on desc.device (= streaming waves of its launch geometry).
int wave_partitions_for(const tkspmv_desc &desc, uint32_t *out, std::string &err);

}  // namespace tkspmv

// The opaque handle of the C ABI (include/tkspmv.h: `typedef struct tkspmv_engine tkspmv_t`). Defined once, here.
struct tkspmv_engine {
    tkspmv::Engine *e;
};
