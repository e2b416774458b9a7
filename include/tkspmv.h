/*
 * tkspmv.h -- C ABI of the MI355X-native Top-K SpMV engine.
 *
 * This is the drop-in boundary for the ONE hot path of AlbertoParravicini/approximate-spmv-topk:
 * "given a fixed sparse matrix A (row-sorted COO, <= 16384 columns) and a fresh dense query x,
 *  return the K rows with the largest A.x".
 *
 * The reference has no FFI; the boundary it re-implements per back-end is the `struct SpMV`
 * engine concept (4 verbs) plus the loader/options helpers every `main` calls. Each entry point
 * below cites the reference interface it replaces (paths relative to the reference repo root):
 *
 *   tkspmv_create        <- SpMV::SpMV + packet_coo + setup   src/fpga/src/host_spmv_bscsr.cpp:104-131,133-321
 *                                                             src/gpu/host_spmv_topk_csr_gpu.cu:95-169
 *   tkspmv_set_query     <- SpMV::reset(vec)                  src/fpga/src/host_spmv_bscsr.cpp:450-485
 *                                                             src/gpu/host_spmv_topk_csr_gpu.cu:241-263
 *   tkspmv_run           <- SpMV::operator()(debug) + wait    src/fpga/src/host_spmv_bscsr.cpp:323-397
 *                                                             src/gpu/host_spmv_topk_csr_gpu.cu:171-231
 *   tkspmv_read          <- SpMV::read_result                 src/fpga/src/host_spmv_bscsr.cpp:399-448
 *                                                             src/gpu/host_spmv_topk_csr_gpu.cu:233-239
 *   tkspmv_mtx_read      <- readMtx / readTuples / mm_read_*  src/common/utils/utils.hpp:372-404,474-520
 *                                                             src/common/utils/mmio.hpp:124-230
 *   tkspmv_sample_vector <- create_sample_vector              src/common/utils/utils.hpp:234-267
 *   tkspmv_options_parse <- Options::Options(argc, argv)      src/common/utils/options.hpp:62-132
 *   tkspmv_generate      <- create_sparse_matrix              src/resources/python/create_matrices.py:58-128
 *
 * Plain pointers and sizes only; no C++/torch types cross this boundary. All functions return a
 * tkspmv_status (0 = OK) unless stated; tkspmv_last_error() returns a thread-local message.
 * The engine NEVER falls back to a CPU path: without a usable HIP device tkspmv_create fails with
 * TKSPMV_ERR_DEVICE.
 */
#ifndef TKSPMV_H
#define TKSPMV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TKSPMV_VERSION 1
#define TKSPMV_MAX_COLS 16384u /* 14 column bits per packed entry (reference MAX_COLS = 1024, types.hpp:55) */
#define TKSPMV_MAX_K 1024      /* reference GPU path: get_topk<<<1,1024>>> => k <= 1024 */

typedef enum {
    TKSPMV_OK = 0,
    TKSPMV_ERR_INVALID = 1,     /* bad argument / descriptor */
    TKSPMV_ERR_NOT_SORTED = 2,  /* COO rows not non-decreasing (reference requires row-major input) */
    TKSPMV_ERR_DEVICE = 3,      /* HIP runtime error or no device */
    TKSPMV_ERR_NOMEM = 4,
    TKSPMV_ERR_IO = 5,          /* file not found / bad MatrixMarket banner */
    TKSPMV_ERR_UNSUPPORTED = 6,
    TKSPMV_ERR_STATE = 7        /* e.g. run before set_query */
} tkspmv_status;

typedef enum {
    TKSPMV_F32 = 0,  /* fp32 values, fp32 x, fp32 accumulate (USE_FLOAT build / GPU hosts) */
    TKSPMV_Q1_7 = 1, /* unsigned fixed point, 1 integer + 7 fraction bits: values, x, products AND sums in 8 bits
                        (the FPGA's ap_ufixed<FIXED_WIDTH,1> real_type with FIXED_WIDTH = 8), see DESIGN.md */
    TKSPMV_Q1_7_WIDE = 2, /* Q1.7 values and products, x block-scaled by a power of two per query, exact (non-wrapping)
                             accumulation: the same 3 B/nnz stream with usable ranking quality */
    TKSPMV_F16 = 3,       /* fp16 values (round to nearest even), fp32 x, fp32 products and sums: 4 B/nnz. The CUDA
                             comparator's half mode (-a, host_spmv_topk_csr_gpu.cu:132-136,152-160) */
    TKSPMV_Q1_7_F32 = 5,  /* BASELINE configs[4] done properly: values stored as Q1.7 bytes (ap_ufixed<8,1,AP_RND,AP_SAT>: rounded
                             to nearest, 3 B/nnz with the column word), x in fp32, fp32 products and sums -- the reduced-
                             precision VALUE STREAM of the FPGA design (fpga_types.hpp:16-23) with the arithmetic of the fp32
                             path. The only error is the quantisation of the values: precision@100 against the fp32 gold 0.97
                             on configs[4] (host_spmv_bscsr.cpp:646-650 is the reference's acceptance metric). Scores are bit-
                             identical to the fp32 engine's on the de-quantised values. */
    TKSPMV_FIXED = 4      /* the FPGA's real_type for any FIXED_WIDTH (types.hpp:20; builds tested by the reference:
                             20/21/25/26/32 bits, test_spmv_topk.py:42-47): ap_ufixed<W,1,AP_TRN_ZERO> with
                             W = desc.fixed_width in [8, 32] -- values, x, every product and every partial sum truncated
                             to W-1 fraction bits, sums wrap at 2.0 (fpga_types.hpp:20,
                             spmv_bscsr_top_k_multicore.hpp:121-141). Values travel as one u32 each (6 B/nnz); ranking and
                             output use the fixed-point score converted to fp32. W = 8 reproduces TKSPMV_Q1_7. */
} tkspmv_precision;

/* Engine variants, the counterpart of the reference's -i/--gpu_impl selector (options.hpp:35, enum GPU_IMPL {CSR,
 * CSR_LIGHTSPMV, COO}: three ways of running the same query on the GPU). All return identical index lists; scores may
 * differ in the last bits (summation order). */
typedef enum {
    TKSPMV_IMPL_STREAM = 0,        /* default: fused streaming kernel over wave-BSCSR packets (batch kernel for sequences) */
    TKSPMV_IMPL_ROW_PER_LANE = 1,  /* one row per lane over the wave-sliced ELL copy (the multi-query kernel with one query
                                      per pass; scores in the gold's summation order). Engines it does not apply to
                                      (reduced precisions, > 1024 columns, ...) run the default. */
    TKSPMV_IMPL_SCORES_SELECT = 2  /* full y = A.x, then an exact radix select over all rows: the structure of the
                                      reference's GPU host (cusparseSpMV + sort, host_spmv_topk_csr_gpu.cu:171-231) */
    /* (3 was rounds 2-4's resident kernel -- one launch serving the reset / run / read loop through pinned memory; since round 4 a launch
       per query through single_kernel is faster on the device and end to end: removed in round 5, tkspmv_create answers TKSPMV_ERR_UNSUPPORTED) */
} tkspmv_impl;

typedef struct tkspmv_engine tkspmv_t;

/* Engine descriptor. Caller owns row/col/val; they are only read during tkspmv_create
 * (the reference keeps raw pointers for the engine lifetime; this engine copies what it needs). */
typedef struct {
    uint32_t rows;            /* logical row count (ids returned are < first_row + rows) */
    uint32_t cols;            /* length of the query vector, <= TKSPMV_MAX_COLS */
    uint64_t nnz;
    const uint32_t *row;      /* [nnz] COO row ids, non-decreasing (reference `x`) */
    const uint32_t *col;      /* [nnz] COO column ids (reference `y`) */
    const float *val;         /* [nnz] values; NULL => all ones (reference -v / ignore_matrix_values) */
    int32_t k;                /* results per query, 1..TKSPMV_MAX_K (reference -k, default 20) */
    int32_t partitions;       /* logical row partitions, reference SPMV_PARTITIONS; 0/1 => one (exact top-k) */
    int32_t k_per_partition;  /* candidates kept per logical partition, reference K (types.hpp:49); 0 => k */
    int32_t precision;        /* tkspmv_precision */
    int32_t device;           /* HIP device ordinal; -1 => current device */
    uint32_t first_row;       /* added to every returned row id (row-sharded multi-GPU) */
    float min_score;          /* rows scoring below this are never returned; gold uses 0 (gold_algorithms.hpp:200) */
    /* tuning knobs, 0 = auto */
    int32_t waves_per_cu;
    int32_t threads_per_wg;
    int32_t nnz_per_lane;     /* 4 or 8 entries per lane per packet; 0 = 4 */
    int32_t stream_replicas;  /* measurement aid: keep R copies of the packet stream in HBM and rotate them per query so
                                 that consecutive queries cannot be served from the 256 MiB Infinity Cache; 0/1 = off */
    int32_t fixed_width;      /* TKSPMV_FIXED: bits per value, 8..32 (0 => 32, the reference's default FIXED_WIDTH,
                                 types.hpp:20); must be 0 for the other precisions */
    int32_t multi_q;          /* queries per matrix pass of tkspmv_enqueue_multi: 0 = off (default), 1, 2, 4 or 8. When set, the
                                 engine keeps a second copy of the matrix in the wave-sliced ELL layout (info.multi_bytes);
                                 info.multi_q tells what the engine uses (8 becomes 4 when k exceeds a quarter of the
                                 threshold groups, 0 when the kernel does not apply) */
    int32_t impl;             /* tkspmv_impl; 0 = default */
    int32_t reserved[1];
} tkspmv_desc;

typedef struct {
    uint32_t rows, cols;
    uint64_t nnz;
    uint64_t packed_entries;      /* nnz + placeholders for empty rows + tail padding */
    uint64_t packed_bytes;        /* bytes of the packet stream + side tables resident in HBM */
    uint64_t algorithmic_bytes;   /* nnz*(sizeof(val)+2) + rows*4 + cols*sizeof(val) + k*8 */
    uint32_t n_packets;
    uint32_t packet_entries;      /* entries per packet = 64 lanes * nnz_per_lane */
    uint32_t n_wave_partitions;   /* physical row ranges: one per wave, or (claim_sets != 0) 8 per claimable set */
    uint32_t packets_per_partition;
    uint32_t grid, block;         /* launch geometry of the streaming kernel */
    uint32_t n_groups;            /* threshold groups publishing maxima */
    uint32_t lds_bytes;
    int32_t k, partitions, k_per_partition, precision, device;
    uint32_t num_cus;
    uint32_t fixed_width;         /* TKSPMV_FIXED: bits per value; 0 otherwise */
    uint32_t multi_q;             /* queries per matrix pass of tkspmv_enqueue_multi; 0 = this engine has no multi-query kernel */
    uint32_t multi_pack_us;       /* tkspmv_create: microseconds spent packing the wave-sliced ELL copy (0 without it) */
    uint64_t multi_bytes;         /* bytes of the wave-sliced ELL copy the multi-query kernel streams (0 without it) */
    uint32_t pack_us;             /* tkspmv_create: microseconds spent packing (on the device: upload of the COO included) */
    uint32_t pack_on_device;      /* 1: the stream was packed by the device packer (default), 0: by the host packer */
    uint32_t claim_sets;          /* always 0 (round 3's dynamically claimed partition sets are gone; the field keeps the layout) */
    uint32_t batch_mode;          /* back-to-back queries: bits 0-7 = selector workgroups of a launch (4 on small matrices), bits 8-15 =
                                     workgroup-local thresholds (0: the device-wide exchange; 1 / 2: see DESIGN.md 3.0b); bits 16-31 = the
                                     n_wave_partitions_hint this engine packed with (tkspmv_pack with the same hint cuts the same partitions) */
    uint64_t state_bytes;         /* device memory of the exchange state of back-to-back queries: the per-query sets (published maxima,
                                     threshold word, one slot per wave, the workgroups' records) and the overflow lists (8 B per row each;
                                     two per engine since round 4, one per query of a launch before) */
    uint64_t batch_stream_bytes;  /* bytes of ONE copy of the packet stream as the batch kernel (tkspmv_enqueue_batch / _many) reads it:
                                     n_packets * batch_packet_bytes. Engines whose fp32 values share their top four bits keep such
                                     copies beside the canonical stream (batch_compact; packed_bytes does not count them): as many
                                     as desc.stream_replicas, at least one */
    uint32_t batch_packet_bytes;  /* bytes of a packet in those copies: 1280 where batch_compact, else the canonical packet's */
    uint32_t batch_compact;       /* 1: the batch kernel streams the stream re-encoded at 5 bytes per entry (option F32_COMPACT) */
} tkspmv_info;

typedef struct {
    double stream_kernel_ns;   /* average hipEvent bracket around the fused streaming kernel (includes event_bracket_ns) */
    double select_kernel_ns;   /* average device time of the final candidate-select kernel */
    double query_ns;           /* average device time per query, back-to-back enqueue (all kernels) */
    double candidates_avg;     /* average number of candidates reaching the select stage */
    double scores_kernel_ns;   /* average device time of the SpMV-only variant (writes the full y; no top-k) */
    double slow_paths_avg;     /* TKSPMV_STATS=1: wave-packets per query that took the candidate path */
    double appended_avg;       /* TKSPMV_STATS=1: rows per query appended to the in-LDS candidate lists */
    double event_bracket_ns;   /* the same event bracket around an empty kernel of the same geometry */
    uint32_t n_queries;
    uint32_t reserved[1];
} tkspmv_timing;

/* ---- engine ------------------------------------------------------------------------------- */
int tkspmv_create(tkspmv_t **out, const tkspmv_desc *desc);
void tkspmv_destroy(tkspmv_t *e);
int tkspmv_get_info(const tkspmv_t *e, tkspmv_info *info);

/* Install a new query vector (host pointer, `cols` floats) -- the reference's reset(vec), host_spmv_bscsr.cpp:354-358. Where the
 * device exposes its memory through a large PCIe BAR (checked by a round trip at create time; option BAR_X) x is stored straight
 * into device memory with CPU stores and a store fence; else it goes through a pinned staging copy and an asynchronous upload.
 * Returns ns in *elapsed_ns if non-NULL. */
int tkspmv_set_query(tkspmv_t *e, const float *host_x, double *elapsed_ns);
/* Same, but x already lives in device memory (no copy; pointer must stay valid until the run completes). */
int tkspmv_set_query_device(tkspmv_t *e, const float *dev_x);

/* Run one query on the current vector and wait. *kernel_ns = device time of the launch(es): where the result travels through
 * host-visible memory (the default) the launch's OWN span -- its s_memrealtime clock, 100 MHz: 10 ns per tick, from the first
 * workgroup's entry to the raising of the result flag; dispatch latency and the instructions behind the flag are outside it --,
 * a hipEvent bracket otherwise (TKSPMV_RUN_EVENTS=1 asks for the bracket; it costs ~6 us around an empty kernel). Engines that
 * stream with workgroup-local thresholds (tkspmv_info.batch_mode bits 8-15) launch single_kernel here; if its selection's
 * check fails -- a query unlike the ones before it -- the query runs again through the exact launch and both spans are added. */
int tkspmv_run(tkspmv_t *e, double *kernel_ns);
/* Enqueue one query on `stream` (hipStream_t cast to void*; NULL => engine stream), no host sync.
 * dev_idx/dev_val: optional device output buffers of k entries (NULL => engine-owned result buffers). */
int tkspmv_enqueue(tkspmv_t *e, const float *dev_x, uint32_t *dev_idx, float *dev_val, void *stream);
/* Enqueue `count` queries back to back (query i uses dev_xs + (i % n_x) * cols), no host sync; the engine-owned
 * result buffers end up holding the last query's top-k. Launch scheme: the batch kernel, up to 32 queries per launch,
 * selections running beside the stream inside the launch (wide x or large k: one launch per query with
 * the selection of query i inside the launch of query i+1 and a small closing launch); on a caller's stream the sequence is
 * complete in stream order when the call returns, on the engine's stream after tkspmv_synchronize (see there). */
int tkspmv_enqueue_many(tkspmv_t *e, const float *dev_xs, int32_t n_x, int32_t count, void *stream);
/* A batch of `count` queries (the loop of the reference's drivers, host_spmv_bscsr.cpp main: for each test vector
 * reset -> operator() -> read_result): query i = dev_xs + i * cols, its k results go to dev_idx + i * k and
 * dev_val + i * k (both NULL => engine-owned buffers, last query wins). Same launch scheme as enqueue_many. */
int tkspmv_enqueue_batch(tkspmv_t *e, const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val,
                         void *stream);
/* Filtered top-k: query i = dev_xs + i * cols, restricted to the rows set in dev_mask + i * mask_stride_words
 * (mask_stride_words = 0: one mask for every query). dev_xs = NULL with count = 1: the vector installed by
 * tkspmv_set_query. dev_mask = NULL: the engine-owned mask installed by tkspmv_set_filter.
 * dev_idx/dev_val: [count][k] or NULL (engine-owned buffers, last query wins). Exact; same stream contract as tkspmv_enqueue_batch.
 * The allow-mask: one bit per local row (before desc.first_row is added), bit r & 31 of word r >> 5 set = row r may be
 * returned; ceil(rows / 32) words per mask, bits at and beyond rows are ignored. The result is exactly the top-k of the
 * allowed rows that have entries and score >= min_score, in the usual order (score descending, then row descending), with
 * scores bit-identical to the unfiltered query's; fewer than k such rows: padded with (0, 0.0f) as tkspmv_read documents.
 * Launch scheme: one exact launch per query (deferred selection, or stream + select, or scores + radix select as the engine
 * would run a single query), never the batch, single-query or multi-query kernels. Errors: TKSPMV_ERR_INVALID for a NULL mask
 * with no filter installed, count < 1 or a negative stride; TKSPMV_ERR_STATE for a NULL dev_xs with no query installed;
 * TKSPMV_ERR_UNSUPPORTED on engines without this path (values other than TKSPMV_F32, the approximate per-partition path). */
int tkspmv_enqueue_filtered(tkspmv_t *e, const float *dev_xs, int32_t count, const uint32_t *dev_mask,
                            int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, void *stream);
/* Host allow-mask (ceil(rows/32) words) copied into an engine-owned device buffer; NULL removes it. Waits for the engine's
 * stream first (a filtered query enqueued there may still read the mask it replaces). */
int tkspmv_set_filter(tkspmv_t *e, const uint32_t *host_mask);
/* Range queries: every row scoring at least a per-query threshold (radius search), where tkspmv_enqueue_filtered answers
 * "the k best". Range query i = dev_xs + i * cols (NULL with count = 1: the vector installed by tkspmv_set_query), threshold
 * dev_thresholds[i] (device array of count floats). dev_mask: optional allow-mask as in tkspmv_enqueue_filtered
 * (NULL: unfiltered; mask_stride_words = 0: one mask for every query). Every row that has entries, is allowed, and
 * scores >= the threshold is a match. dev_counts[i] (required) = number of matches, also when it exceeds capacity;
 * dev_idx / dev_val + i * capacity (both NULL with capacity = 0: count only) receive min(count, capacity) distinct
 * matches -- row id + desc.first_row, and the score, bit-identical to the score every other path reports for that
 * row -- in NO particular order; which matches are kept when count > capacity is unspecified. Entries beyond
 * min(count, capacity) are not written. Any float is a threshold: -inf returns every row that has entries, NaN matches
 * nothing; desc.min_score plays no part. Complete in stream order on any stream; reads and writes no engine state (no result
 * buffer, no carried threshold), so it may be mixed freely with the other calls. Errors: TKSPMV_ERR_UNSUPPORTED where
 * tkspmv_enqueue_filtered reports it; TKSPMV_ERR_INVALID for count < 1, NULL thresholds or counts, a negative stride, one of
 * dev_idx / dev_val NULL and not the other, capacity > 0 with NULL outputs or capacity = 0 with outputs, NULL dev_xs with
 * count != 1; TKSPMV_ERR_STATE for a NULL dev_xs with no query installed. */
int tkspmv_enqueue_range(tkspmv_t *e, const float *dev_xs, int32_t count, const float *dev_thresholds,
                         const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                         uint32_t capacity, uint32_t *dev_counts, void *stream);
/* The host-side counterpart (reset -> run -> read in one call): the installed query vector, a host threshold, the
 * mask installed by tkspmv_set_filter when use_filter != 0; waits; idx/val (host, capacity entries) receive the
 * matches SORTED like tkspmv_read (score descending, row descending); *count = number of matches (also beyond capacity;
 * min(*count, capacity) entries are written). TKSPMV_ERR_INVALID for use_filter with no filter installed. */
int tkspmv_run_range(tkspmv_t *e, float threshold, int32_t use_filter, uint32_t *idx, float *val,
                     uint32_t capacity, uint64_t *count);
/* Facet counts (aggregation): of the rows that match a range query, how many carry each label, and which is each label's best
 * hit -- facet counts beside a result list, hit counts per tenant or shard, class histograms of a labelled corpus --, without
 * writing the matches themselves: the answer is n_bins words per query, accumulated where the matches are found (facet_kernel:
 * range_kernel's streaming loop with a histogram for a sink). Query i, dev_xs, dev_thresholds[i], dev_mask / mask_stride_words:
 * exactly as in tkspmv_enqueue_range, and a row MATCHES exactly as there: it has entries, is allowed by the mask, and its fp32
 * score -- the bits every other path reports -- is >= the threshold compared as floats (-inf: every row with entries; NaN:
 * nothing; desc.min_score plays no part).
 * dev_labels: device array of `rows` labels, one per LOCAL row, one array for every query of the call; a row whose label is
 * >= n_bins belongs to no bin (0xFFFFFFFF: "no facet") and still counts in the total. dev_labels = NULL: the labels installed
 * by tkspmv_set_groups; n_bins must then be 0 and the engine's n_groups is used.
 * Outputs of query i: dev_counts[i * n_bins + b] (required) = matches with label b. dev_best[i * n_bins + b] (optional) = the
 * bin's match that comes first in the result order (order key of the score descending, then global row id descending: the
 * maximum of order key << 32 | first_row + row): row = its global id, score_bits = its score's bits; an empty bin gives {0, 0},
 * which dev_counts tells apart from "row 0 scoring +0.0f". dev_totals[i] (optional) = all matches, those of no bin included:
 * what tkspmv_enqueue_range puts into dev_counts[i]. Exactly count * n_bins entries of dev_counts and of dev_best and count of
 * dev_totals are written, nothing else. Bit-reproducible from run to run: counts are integers, the best is a maximum.
 * Stream and state contract: tkspmv_enqueue_range's -- complete in stream order on any stream; reads and writes no result
 * buffer, exchange set, record, verdict, carried threshold or launch counter and no engine-owned scratch, so any number of calls
 * may be in flight and it may be mixed freely with every other call. (With dev_labels = NULL the installed labels are read:
 * tkspmv_set_groups waits for the engine's stream only.) The call zeroes its outputs in stream order, streams the matrix once
 * per query (launches of up to 32 queries) and, with dev_best, ends with one small launch over count * n_bins entries.
 * Calls of few bins (option FACET_LDS_BINS; by default up to 4096 bins, 512 above 4096 columns) collect in a histogram per
 * workgroup in LDS that is added to the outputs once per query; calls of more bins update the outputs with global atomics.
 * Errors, checked before any device call: TKSPMV_ERR_INVALID for a NULL engine, NULL thresholds or counts, count < 1, a negative
 * stride, dev_xs = NULL with count != 1, dev_labels given with n_bins = 0, dev_labels = NULL with n_bins != 0, n_bins > 2^30,
 * a dev_best that is not 8-byte aligned; TKSPMV_ERR_STATE for a NULL dev_xs with no vector installed or NULL dev_labels with no
 * labels installed; TKSPMV_ERR_UNSUPPORTED exactly where tkspmv_enqueue_range reports it. */
typedef struct { uint32_t row; uint32_t score_bits; } tkspmv_facet_best;   /* 8 bytes, 8-byte aligned */
int tkspmv_enqueue_facets(tkspmv_t *e, const float *dev_xs, int32_t count, const float *dev_thresholds,
                          const uint32_t *dev_mask, int64_t mask_stride_words,
                          const uint32_t *dev_labels, uint32_t n_bins,
                          uint32_t *dev_counts, tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream);
/* The host-side counterpart: the installed query vector, a host threshold, the labels installed by tkspmv_set_groups, the mask
 * installed by tkspmv_set_filter when use_filter != 0 (TKSPMV_ERR_INVALID if none is); runs on engine-owned scratch that grows
 * to n_groups entries, and waits. counts[n_groups] and best[n_groups] (host; either may be NULL) and *total receive the result. */
int tkspmv_run_facets(tkspmv_t *e, float threshold, int32_t use_filter,
                      uint32_t *counts, tkspmv_facet_best *best, uint64_t *total);
/* Boolean term predicates: an allow-mask made on the device from the rows' own columns -- "only rows that contain column 17 and one
 * of {40, 41}, and not column 900", or a term's document frequency -- where tkspmv_set_filter takes a mask the host built. The
 * kernel (match_kernel) streams the packets' column plane alone: the values never travel.
 * Clause table: `cols` u32 words; bit c of word j set = column j belongs to clause c (c in 0..31). A clause is a set of columns; a
 * row satisfies it when it has an entry in any of them. Query i uses dev_clauses + i * clause_stride_words (0: one table for every
 * query; else >= cols).
 * Row word: W(r) = the OR of table[col] over the stored entries of local row r. An entry is an entry of the COO the engine was
 * created from, whatever its value (an explicit 0.0 counts, so does a negative value; a column that occurs several times changes
 * nothing); placeholders of empty rows and the padding behind a partition's last row are not entries.
 * Row r MATCHES predicate dev_preds[i] when it has entries, is allowed by the optional dev_mask (dev_mask / mask_stride_words exactly
 * as in tkspmv_enqueue_range; NULL: unfiltered), (W & must) == must, (W & must_not) == 0 and popcount(W & should) >= min_should.
 * All-zero fields match every row that has entries; min_should > popcount(should) matches nothing. desc.min_score and
 * desc.first_row play no part: the mask is over local rows, like every allow-mask.
 * Outputs of query i: the mask, words = max(1, ceil(rows / 32)) words at dev_out + i * out_stride_words (dev_out required;
 * out_stride_words >= words, or 0 with count = 1): bit r & 31 of word r >> 5 is set if and only if row r matches. All `words` words
 * are written and bits at and beyond `rows` are 0, so the result is valid wherever a mask is accepted; words between the masks of a
 * strided output are not written. dev_out must not overlap dev_mask. dev_counts[i] (optional) = the number of matching rows.
 * Exact and bit-reproducible: a pure function of the matrix's sparsity pattern.
 * Stream and state contract: tkspmv_enqueue_range's -- complete in stream order on any stream (NULL: the engine's); reads the
 * matrix, the table, the predicates and the mask and writes its two outputs; touches no result buffer, exchange set, record,
 * verdict, carried threshold, launch counter or engine scratch, so any number of calls may be in flight and it mixes freely with
 * every other call. Query i reads stream copy i % stream_replicas. In stream order the result feeds tkspmv_enqueue_filtered,
 * _range, _facets, _grouped and _after with no host round trip. The call zeroes its outputs in stream order and streams the column
 * plane once per query (launches of up to 32 queries).
 * Errors, checked before any device call: TKSPMV_ERR_INVALID for a NULL engine, table, predicates or output, count < 1, a negative
 * stride, a clause stride that is neither 0 nor >= cols, an output stride below `words` (except 0 with count = 1);
 * TKSPMV_ERR_UNSUPPORTED exactly where tkspmv_enqueue_row_vectors reports it (a packet stream that is not fp32, an engine that does
 * not hold the packets) -- the approximate per-partition engines are served -- and, with dev_mask, where tkspmv_enqueue_filtered
 * reports it. */
typedef struct { uint32_t must, must_not, should, min_should; } tkspmv_match;   /* 16 bytes */
int tkspmv_enqueue_match(tkspmv_t *e, const uint32_t *dev_clauses, int64_t clause_stride_words,
                         const tkspmv_match *dev_preds, int32_t count,
                         const uint32_t *dev_mask, int64_t mask_stride_words,
                         uint32_t *dev_out, int64_t out_stride_words, uint32_t *dev_counts, void *stream);
/* The host-side counterpart: a host table (cols words) and a host predicate, the mask installed by tkspmv_set_filter when
 * use_filter != 0 (TKSPMV_ERR_INVALID if none is); runs on engine-owned scratch allocated on the first call, and waits.
 * host_mask (`words` words) and *count may each be NULL. install != 0: the result becomes the engine's installed filter, as
 * tkspmv_set_filter would install it, by a device-to-device copy; with use_filter as well, the new filter is the old one AND the
 * predicate. */
int tkspmv_run_match(tkspmv_t *e, const uint32_t *host_clauses, const tkspmv_match *pred,
                     int32_t use_filter, int32_t install, uint32_t *host_mask, uint64_t *count);
/* Grouped top-k (result collapsing): the k best GROUPS of rows, each shown once by its best row -- the k best documents by
 * their best passage, products by their best variant. Every local row carries a label group[r] < n_groups, a property of the
 * index like the allow-mask. For a query a row is ELIGIBLE when it has entries, is allowed by the optional allow-mask, and its
 * score passes desc.min_score as the engine's exact selection decides it (order key >= the key of min_score, score > -inf). A
 * group's REPRESENTATIVE is its eligible row that comes first in the result order (score descending, then row id descending); a
 * group without an eligible row does not exist for that query. The result is the first k representatives in that same order:
 * the engine's complete ranking of the eligible rows with every row dropped whose group already appeared, cut at k. Hence
 * group[r] = r gives the engine's exact top-k bit for bit, and one group gives the query's best row alone.
 *
 * host_groups: [rows] labels, checked on the host (TKSPMV_ERR_INVALID for n_groups = 0 or a label >= n_groups: nothing is
 * installed, earlier labels stay); NULL removes them. Waits for the engine's stream first, as tkspmv_set_filter does (a grouped
 * query on a caller's stream must have been waited for by the caller), and allocates the path's scratch: 8 bytes per row and
 * 24 bytes per group. */
int tkspmv_set_groups(tkspmv_t *e, const uint32_t *host_groups, uint32_t n_groups);
/* Grouped query i = dev_xs + i * cols (NULL with count = 1: the vector installed by tkspmv_set_query). dev_mask /
 * mask_stride_words: as in tkspmv_enqueue_filtered, but NULL means UNFILTERED. dev_idx / dev_val / dev_grp: [count][k], all
 * three given or all three NULL (engine-owned buffers, last query wins; tkspmv_read then sees idx / val). Entry j of a list:
 * the representative's row id + desc.first_row, its score with the bits every other path reports for that row, its group id.
 * Fewer than k groups exist: the tail is padded with (0, 0.0f) as tkspmv_read documents, with group id 0xFFFFFFFF. dev_n:
 * [count] or NULL, the number of real entries of each list (a pad and "row 0 scoring +0.0f" differ in the group id and here).
 * Exact, and bit-reproducible: a group's representative is a maximum, which does not depend on the order rows arrive in.
 * Every value type is served without a mask; a mask needs the filtered path's kernels (TKSPMV_F32).
 * Stream contract: complete in stream order on any stream. The call uses scratch owned by the engine, so two grouped calls
 * must NOT be in flight on two streams at once. It reads and writes no exchange state, carried threshold, verdict or deferred
 * selection, so it may be mixed freely with the other calls on one stream; with engine-owned outputs it first settles pending
 * checks of earlier batch launches, as tkspmv_enqueue_filtered does.
 * Launch scheme per query: the SpMV-only kernel (every row's score), one pass that folds rows into their group's best
 * (score, row) key, a radix select over the groups, the selection kernel over the selected groups' representatives.
 * Errors: TKSPMV_ERR_INVALID for count < 1, a negative stride, output pointers partly given; TKSPMV_ERR_UNSUPPORTED on the
 * approximate per-partition engines, on engines that do not hold the packet stream, and for a mask where
 * tkspmv_enqueue_filtered reports it; TKSPMV_ERR_STATE with no labels installed or a NULL dev_xs with no query installed. */
int tkspmv_enqueue_grouped(tkspmv_t *e, const float *dev_xs, int32_t count, const uint32_t *dev_mask,
                           int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp,
                           uint32_t *dev_n, void *stream);
/* The host-side counterpart: the installed query vector, the mask installed by tkspmv_set_filter when use_filter != 0
 * (TKSPMV_ERR_INVALID if none is); waits; idx / val / grp (host, k entries each, any may be NULL) receive the list, *n the
 * number of real entries. */
int tkspmv_run_grouped(tkspmv_t *e, int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n);
/* Search-after paging: "the next k". The result order is a strict total order -- score descending by order key, then row id
 * descending: a 64-bit integer comparison of (order key << 32 | global row id), no float is compared as a float --, so "every
 * eligible row that ranks strictly behind entry (row, score)" is well defined, stateless and exact across ties. A cursor is such a
 * position and nothing more: it need not name a row of this engine (a masked row, an empty row, a row of another shard, a score
 * no row has are all fine). START cuts nothing, END cuts everything. A row is ELIGIBLE exactly as in the grouped call: it has
 * entries, is allowed by the optional mask, its order key is at least the key of desc.min_score and its score is above -inf. It
 * ranks behind an AFTER cursor when order_key(score) < order_key(cursor score), or the keys are equal and first_row + local row <
 * cursor.row. NaN scores and NaN cursor scores have no stated contract. */
typedef struct { uint32_t row; uint32_t score_bits; uint32_t state; uint32_t reserved; } tkspmv_cursor; /* 16 bytes */
/* state: 0 = TKSPMV_CURSOR_START (from the top; row / score_bits ignored), 1 = TKSPMV_CURSOR_AFTER, 2 = TKSPMV_CURSOR_END; any other value acts as END */
#define TKSPMV_CURSOR_START 0u
#define TKSPMV_CURSOR_AFTER 1u
#define TKSPMV_CURSOR_END 2u
/* Query i = dev_xs + i * cols (NULL with count = 1: the vector installed by tkspmv_set_query). dev_cursors: [count] cursors in
 * DEVICE memory, query i reads dev_cursors[i] when its turn comes in stream order; NULL: START for every query. dev_mask /
 * mask_stride_words: as in tkspmv_enqueue_grouped (NULL: unfiltered). Outputs of query i:
 *   dev_idx / dev_val + i * k: the first k eligible rows behind the cursor in the usual order, global ids, the score bits every
 *     other path reports; a short list is padded with (0, 0.0f). Both given or both NULL (the engine-owned pair, the last query
 *     wins, tkspmv_read sees it; pending checks of trusted batch launches are then settled first, as tkspmv_enqueue_grouped does).
 *   dev_n[i] (optional): the number of real entries.
 *   dev_total[i] (optional): the eligible rows behind the cursor, the returned ones included -- the "hits left".
 *   dev_next[i] (optional): the cursor of the following page: AFTER(the last real entry) when total > k, END otherwise (n = 0
 *     included), so a loop "while state != END" ends without an empty trailing page. dev_next may be dev_cursors itself: the
 *     cursor is read at the start of query i and written at its end, in stream order, so P calls with one buffer walk P pages
 *     with no host round trip.
 * Hence with START the list is the engine's exact top-k bit for bit, and the pages concatenated are the engine's complete ranking
 * of the eligible rows. Row-sharded use: give every shard the SAME cursor (ids are global), merge the shards' pages with
 * tkspmv_merge_topk; the next cursor is AFTER(the last real merged entry) when the shards' totals sum to more than k, else END (a
 * shard's own dev_next is not the global one).
 * Stream contract (the grouped call's): complete in stream order on any stream; reads and writes no exchange set, record, verdict,
 * carried threshold or deferred selection; the scratch belongs to the engine, so only ONE such call may be in flight at a time
 * (tkspmv_enqueue_boosted runs on the same scratch: the rule covers both kinds of call together). The
 * FIRST call allocates that scratch, about 12 bytes per row (the scores and a candidate list that holds every tie at the cut).
 * Launch scheme per query: the SpMV-only kernel, one pass that cuts at the cursor and counts (after_cut_kernel), the radix select,
 * the selection kernel, one small block for n / total / next.
 * Errors: TKSPMV_ERR_INVALID, before any device call, for a NULL engine, count < 1, a negative stride, dev_idx / dev_val partly
 * given, dev_xs = NULL with count != 1; TKSPMV_ERR_STATE for dev_xs = NULL with no vector installed; TKSPMV_ERR_UNSUPPORTED where
 * tkspmv_enqueue_grouped reports it (approximate per-partition engines, engines that do not hold the packet stream, a mask on
 * engines without the filtered path's kernels). Every value type is served without a mask. */
int tkspmv_enqueue_after(tkspmv_t *e, const float *dev_xs, int32_t count, const tkspmv_cursor *dev_cursors,
                         const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                         uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream);
/* The host-side counterpart: the installed query vector, a HOST cursor (NULL: START), the mask installed by tkspmv_set_filter when
 * use_filter != 0 (TKSPMV_ERR_INVALID if none is); waits; idx / val (host, k entries each), *n, *total and *next receive the page
 * (any may be NULL). */
int tkspmv_run_after(tkspmv_t *e, const tkspmv_cursor *cursor /* host, NULL = START */, int32_t use_filter,
                     uint32_t *idx, float *val, int32_t *n, uint32_t *total, tkspmv_cursor *next);
/* Boosted top-k (a "function score"): search-after pages over a per-row transform of the score. With s the fp32 score every other
 * path reports for LOCAL row r (weight and bias are indexed like masks and group labels),
 *     t  = weight ? weight[r] * s : s
 *     s' = bias   ? t + bias[r]   : t
 * as two separately rounded fp32 operations (__fmul_rn, __fadd_rn: never one fma; fp32 subnormals are kept, in products and sums
 * alike, on the device as in the host restatement). A row whose score is -inf -- it has no entries, or the mask excludes it --
 * stays -inf whatever weight and bias say; a row whose s' is not finite (NaN, +inf, -inf) is not eligible. Everything else is
 * tkspmv_enqueue_after's contract read on s': eligible = order key of s' >= order key of desc.min_score; the order = order key of s'
 * descending, then global row id descending; a cursor's score_bits are a boosted score; n / total / next, the pads (0, 0.0f) and the
 * row-sharded recipe (the same cursor for every shard, global ids, each shard its own slice of weight and bias) are unchanged. Hence
 * weight = all 1.0f without a bias, and bias = all -0.0f without a weight, give tkspmv_enqueue_after's lists bit for bit (a bias
 * of +0.0f does not: it turns a score of -0.0f into +0.0f). Uses: static priors (s + b[r]), demotions (w[r] * s), cosine instead of
 * the dot product (w[r] = 1 / |row r|, no re-packing), exact hybrid fusion with a per-query bias (sparse score + alpha * dense
 * score[r]: the top-k of the SUM over all rows), bottom-k (w = -1 with desc.min_score = -inf).
 * tkspmv_set_boost installs a pair of HOST arrays of desc.rows floats each in engine-owned device memory (freed by
 * tkspmv_destroy); either may be NULL (no multiply / no add), both NULL removes the installed boost. An entry that is not finite
 * gives TKSPMV_ERR_INVALID and installs nothing: the boost installed before stays. The call waits for the engine's stream. */
int tkspmv_set_boost(tkspmv_t *e, const float *host_weight, const float *host_bias);
/* tkspmv_enqueue_after with a boost: query i reads dev_weight + i * boost_stride and dev_bias + i * boost_stride (DEVICE arrays
 * of desc.rows floats, the stride in floats, 0 = one pair for every query; no alignment is required: 16-byte loads are used where
 * pointer and stride allow them). One of the two may be NULL (no multiply / no add); BOTH NULL names the boost tkspmv_set_boost
 * installed. Every other argument, dev_next == dev_cursors and the engine-owned outputs for dev_idx = dev_val = NULL included, is
 * exactly tkspmv_enqueue_after's.
 * Stream contract: tkspmv_enqueue_after's. The call runs on the search-after path's scratch (allocated by the first call of either
 * kind), so "only ONE such call in flight at a time" covers tkspmv_enqueue_after and tkspmv_enqueue_boosted TOGETHER. No exchange
 * set, record, verdict, carried threshold or deferred selection is read or written.
 * Launch scheme per query: the SpMV-only kernel, ONE pass that transforms, cuts at the cursor and counts (boost_cut_kernel, in
 * after_cut_kernel's place: no launch is added), the radix select, the selection kernel, one small block for n / total / next.
 * Errors, in this order: TKSPMV_ERR_INVALID, before any device call, for a NULL engine, count < 1, a negative boost_stride or
 * mask_stride_words, dev_idx / dev_val partly given, dev_xs = NULL with count != 1; TKSPMV_ERR_UNSUPPORTED where
 * tkspmv_enqueue_after reports it; TKSPMV_ERR_STATE for both arrays NULL with no boost installed, or dev_xs = NULL with no vector
 * installed. Every value type is served without a mask. Range, facet and grouped queries over s': tkspmv_enqueue_boosted_range,
 * tkspmv_enqueue_boosted_facets, tkspmv_enqueue_boosted_grouped below. */
int tkspmv_enqueue_boosted(tkspmv_t *e, const float *dev_xs, int32_t count,
                           const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                           const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words,
                           uint32_t *dev_idx, float *dev_val, uint32_t *dev_n, uint32_t *dev_total,
                           tkspmv_cursor *dev_next, void *stream);
/* tkspmv_run_after with the installed boost (TKSPMV_ERR_STATE if none is installed). */
int tkspmv_run_boosted(tkspmv_t *e, const tkspmv_cursor *cursor /* host, NULL = START */, int32_t use_filter,
                       uint32_t *idx, float *val, int32_t *n, uint32_t *total, tkspmv_cursor *next);
/* Boosted range, facet and grouped queries: thresholds, counts and groups on the boosted score. The match rule is one for all three.
 * With s' = tkspmv_enqueue_boosted's boosted score of LOCAL row r (above: two separately rounded operations; a row that holds -inf
 * stays -inf; an s' that is not finite becomes -inf), a row whose s' is -inf takes part in nothing: it is no match, is not counted,
 * is not eligible and never a representative. dev_weight, dev_bias and boost_stride are tkspmv_enqueue_boosted's: device arrays by
 * local row, either may be NULL, BOTH NULL names the installed boost, the stride in floats (0 = one pair for every query), no
 * alignment required. They stand behind `count`; every other argument is the base call's.
 * Why not inside range_kernel / facet_kernel: their per-packet trigger bounds RAW row sums, so a boosted threshold has to score every
 * row. Per query, on the caller's stream: the SpMV-only kernel into an engine-owned score array (through the filtered kernel when
 * there is a mask), then ONE pass over that array which transforms, compares and delivers (boosted_hits_kernel, boosted_bins_kernel);
 * the array is read only. The grouped form runs boost_cut_kernel (no cursor) over the grouped path's array, then that path unchanged.
 * Stream contract: the scratch is the engine's. tkspmv_enqueue_after, tkspmv_enqueue_boosted, tkspmv_enqueue_boosted_range and
 * tkspmv_enqueue_boosted_facets share the search-after path's scratch (the first call of any of them allocates it, about 12 bytes per
 * row): only ONE call of these four kinds may be in flight at a time, TOGETHER. tkspmv_enqueue_boosted_grouped counts together with
 * tkspmv_enqueue_grouped in the same way. No exchange set, record, verdict, carried threshold or deferred selection is read or
 * written.
 * Errors, in tkspmv_enqueue_boosted's order: TKSPMV_ERR_INVALID, before any device call, for what the base call rejects, a negative
 * boost_stride, or dev_xs = NULL with count != 1; TKSPMV_ERR_UNSUPPORTED where tkspmv_enqueue_grouped reports it (so every value
 * type is served without a mask, fp32 with one, and the approximate per-partition engines are refused); TKSPMV_ERR_STATE for both
 * arrays NULL with no boost installed, dev_xs = NULL with no vector installed, or no labels.
 *
 * tkspmv_enqueue_boosted_range extends tkspmv_enqueue_range: row r matches query i when s' > -inf and s' >= dev_thresholds[i],
 * compared as floats (a threshold of -inf returns every row with a finite s', NaN nothing; desc.min_score plays no part).
 * dev_counts[i] is the number of matches, also beyond capacity; the first min(count, capacity) distinct matches are written as
 * (first_row + r, s') in no particular order, nothing beyond them. */
int tkspmv_enqueue_boosted_range(tkspmv_t *e, const float *dev_xs, int32_t count,
                                 const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                 const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words,
                                 uint32_t *dev_idx, float *dev_val, uint32_t capacity, uint32_t *dev_counts, void *stream);
/* tkspmv_run_range with the installed boost (TKSPMV_ERR_STATE if none is installed): the matches sorted like tkspmv_run_range's. */
int tkspmv_run_boosted_range(tkspmv_t *e, float threshold, int32_t use_filter, uint32_t *idx, float *val,
                             uint32_t capacity, uint64_t *count);
/* tkspmv_enqueue_boosted_facets extends tkspmv_enqueue_facets: the same match rule; dev_counts, dev_best and dev_totals are exactly
 * tkspmv_enqueue_facets' (dev_best: the maximum of order key of s' << 32 | global row, as {row, bits of s'}; labels >= n_bins count
 * in the total only; {0, 0} for an empty bin). Calls of at most min(option FACET_LDS_BINS, 4096) bins are counted in a
 * workgroup-private histogram in LDS, calls of more bins with global atomics. */
int tkspmv_enqueue_boosted_facets(tkspmv_t *e, const float *dev_xs, int32_t count,
                                  const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                  const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words,
                                  const uint32_t *dev_labels, uint32_t n_bins, uint32_t *dev_counts,
                                  tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream);
/* tkspmv_run_facets with the installed boost (TKSPMV_ERR_STATE if none is installed). */
int tkspmv_run_boosted_facets(tkspmv_t *e, float threshold, int32_t use_filter,
                              uint32_t *counts, tkspmv_facet_best *best, uint64_t *total);
/* tkspmv_enqueue_boosted_grouped extends tkspmv_enqueue_grouped: a row is eligible when the order key of s' is at least that of
 * desc.min_score and s' > -inf; the representative, the order and the returned value are all on s'. Pads, dev_grp and dev_n are
 * unchanged, and so are the engine-owned outputs for dev_idx = dev_val = dev_grp = NULL. */
int tkspmv_enqueue_boosted_grouped(tkspmv_t *e, const float *dev_xs, int32_t count,
                                   const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                   const uint32_t *dev_mask, int64_t mask_stride_words,
                                   uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp, uint32_t *dev_n, void *stream);
/* tkspmv_run_grouped with the installed boost (TKSPMV_ERR_STATE if none is installed). */
int tkspmv_run_boosted_grouped(tkspmv_t *e, int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n);
/* Queries by stored row ("which rows are closest to row r?": more-like-this, de-duplication, the k-NN self-join A.A^T top-n --
 * the product the reference's CPU comparator sparse_dot_topn exists for). dev_rows[i] is a GLOBAL row id (desc.first_row + local
 * row): exactly what queries return, so results can be fed back. dev_xs + i * cols receives row i as the dense vector of cols
 * floats that every tkspmv_enqueue_* call takes: zeros, and at each column of the row the fp32 sum of the row's entries with that
 * column, added in stream order starting from +0.0f (a column may occur several times in a row) -- the vector for which A.x means
 * "similarity to row r". dev_len[i] (dev_len may be NULL) receives the row's number of entries: 0 for a row without entries (a zero
 * vector), 0xFFFFFFFF for an id outside [first_row, first_row + rows) (a zero vector as well). The same id may occur any number of
 * times. Asynchronous, complete in stream order on any stream (NULL: the engine's); reads and writes no engine state, so it may be
 * mixed freely with the other calls, as tkspmv_enqueue_range may; stream copy 0 of the matrix is read (desc.stream_replicas plays no
 * part). One wave per row (row_vectors_kernel): the row is found by bisecting the packets' row table.
 * Errors: TKSPMV_ERR_INVALID for a NULL engine, dev_rows or dev_xs or count < 1 (checked before any device call);
 * TKSPMV_ERR_UNSUPPORTED when the engine's packet stream is not fp32 (reduced-precision and fixed-point values) or the engine does
 * not hold the packets. The approximate per-partition engines ARE served: extraction does not depend on how rows are selected. */
int tkspmv_enqueue_row_vectors(tkspmv_t *e, const uint32_t *dev_rows, int32_t count, float *dev_xs, uint32_t *dev_len, void *stream);
/* The same with host arrays (host_xs: [count][cols], host_len: [count] or NULL); waits. */
int tkspmv_row_vectors(tkspmv_t *e, const uint32_t *host_rows, int32_t count, float *host_xs, uint32_t *host_len);
/* For every given row (global ids, host array) the engine's top-k with that row as the query: idx / val are [count][k] host
 * arrays, each list ordered as tkspmv_read orders it and final when the call returns. Works in chunks of at most 1024 rows and
 * 64 MiB of vectors on engine-owned scratch: ids up, row vectors, the launch path of tkspmv_enqueue_batch, tkspmv_synchronize,
 * results down. exclude_self != 0: the entry whose id is the query's own row is removed from its list on the host -- the rest
 * moves up, the last slot becomes the pad (0, 0.0f); a list without the row is unchanged. To get k others, create the engine
 * with k + 1. Errors as above (idx and val must be given). */
int tkspmv_run_similar(tkspmv_t *e, const uint32_t *host_rows, int32_t count, int32_t exclude_self, uint32_t *idx, float *val);
/* Scores of given rows ("what do these rows score for this query?": rescoring candidates that came from elsewhere -- a dense index,
 * another shard, a cached page --, fusing sparse and dense scores, evaluating labelled (query, row) pairs, pairwise similarities
 * with tkspmv_enqueue_row_vectors supplying the vectors). Query q is dev_xs + q * cols (dev_xs = NULL with count = 1: the vector
 * installed by tkspmv_set_query, ordered as tkspmv_enqueue_range orders it); its list is dev_rows + q * rows_stride, n_rows GLOBAL
 * row ids (desc.first_row + local row: what queries return; rows_stride = 0: one list for every query; the same id may occur any
 * number of times). dev_scores[q * n_rows + i] receives the score of row dev_rows[q * rows_stride + i] for query q: exactly
 * count * n_rows floats are written, nothing else. The score is the fp32 value every other path reports for that row and query,
 * bit for bit -- tkspmv_scores' y[row], what tkspmv_enqueue_range stores, what the top-k lists carry: it is computed from the row's
 * own packets with the streaming kernels' arithmetic (score_rows_kernel: the row is found by bisecting the packets' row table, a
 * wave per list entry), so the matrix is not streamed. A row without entries scores +0.0f, an id outside
 * [first_row, first_row + rows) -inf (bits 0xFF800000: it sorts last in a rerank); desc.min_score plays no part. Asynchronous,
 * complete in stream order on any stream (NULL: the engine's); reads stream copy 0 and writes dev_scores only: no engine state is
 * touched, so it may be mixed freely with the other calls, as tkspmv_enqueue_range may.
 * Errors: TKSPMV_ERR_INVALID (checked before any device call) for a NULL engine, dev_rows or dev_scores, count < 1, n_rows < 1, a
 * negative rows_stride or one that is neither 0 nor >= n_rows, dev_xs = NULL with count != 1; TKSPMV_ERR_STATE for dev_xs = NULL
 * with no vector installed; TKSPMV_ERR_UNSUPPORTED when the engine's packet stream is not fp32 (reduced-precision and fixed-point
 * values) or the engine does not hold the packets. Served wherever tkspmv_enqueue_row_vectors is, the approximate per-partition
 * engines included. */
int tkspmv_enqueue_score_rows(tkspmv_t *e, const float *dev_xs, int32_t count, const uint32_t *dev_rows, int32_t n_rows, int64_t rows_stride,
                              float *dev_scores, void *stream);
/* The same with host arrays (host_xs = NULL with count = 1: the installed vector); waits. Works in chunks of at most 1024 queries,
 * 64 MiB of vectors and 16384 list entries per query on engine-owned scratch. */
int tkspmv_score_rows(tkspmv_t *e, const float *host_xs, int32_t count, const uint32_t *host_rows, int32_t n_rows, int64_t rows_stride,
                      float *host_scores);
/* Row statistics ("how long is every row?": the norms cosine similarity and length normalisation divide by), taken from the matrix
 * the engine already holds -- what host.cosine_weights of the Python package computes from the COO on the host, for engines that no
 * longer have a COO (tkspmv_create_packed, a shard that dropped its slice). dev_out[r] receives one float32 for LOCAL row r
 * (indexed like masks, group labels, weight and bias); exactly desc.rows floats are written:
 *   TKSPMV_ROW_NNZ     the row's stored entries as the packer stored them (explicit zeros and repeated columns count), exact below
 *                      2^24 entries per row: what tkspmv_enqueue_row_vectors reports in dev_len and tkspmv_packed_get_row in *n
 *   TKSPMV_ROW_L1      the sum of |v| over the row's entries
 *   TKSPMV_ROW_L2SQ    the sum of v * v, each product one separately rounded fp32 multiplication
 *   TKSPMV_ROW_INV_L2  the cosine weight 1.0f / sqrt(L2SQ): two separately rounded IEEE fp32 operations, subnormals kept; +0.0f where
 *                      L2SQ is 0, +inf or NaN, so every weight is finite
 * The sums are formed in the order every streaming path sums a row's score in (in-lane segmented sums, the clipped scan over the 64
 * lanes, the packet carry): a statistic is, bit for bit, the score the row would get if every product were |v| or v * v, so it is
 * reproducible and tkspmv_packed_row_stats restates it on the host. A row without entries gives +0.0f for every kind.
 * desc.min_score, the installed filter and the installed query play no part. One pass over stream copy 0 of the matrix
 * (row_stats_kernel), with one 4-byte store per row behind a memset of dev_out on the same stream. Asynchronous, complete in stream
 * order on any stream (NULL: the engine's); reads and writes no engine state, so it may be mixed freely with the other calls, as
 * tkspmv_enqueue_range may. With desc.rows = 0 the call succeeds and writes nothing.
 * Per-query or combined weights: take TKSPMV_ROW_INV_L2 or TKSPMV_ROW_NNZ into a device array of your own, compute what you need
 * there and pass it as dev_weight to tkspmv_enqueue_boosted -- pivoted length normalisation, for one, is
 * weight[r] = 1 / (1 - b + b * nnz[r] / avg) with avg the mean of nnz.
 * Errors: TKSPMV_ERR_INVALID (checked before any device call) for a NULL engine, a NULL dev_out or a kind outside 0 .. 3;
 * TKSPMV_ERR_UNSUPPORTED exactly where tkspmv_enqueue_row_vectors reports it (a packet stream that is not fp32, an engine that does
 * not hold the packets). The approximate per-partition engines ARE served. */
#define TKSPMV_ROW_NNZ 0
#define TKSPMV_ROW_L1 1
#define TKSPMV_ROW_L2SQ 2
#define TKSPMV_ROW_INV_L2 3
int tkspmv_enqueue_row_stats(tkspmv_t *e, int32_t kind, float *dev_out /* [rows] */, void *stream);
/* The same into a host array of desc.rows floats, on engine-owned scratch of that size (allocated by the first call); waits for its
 * own launch only. */
int tkspmv_row_stats(tkspmv_t *e, int32_t kind, float *host_out /* [rows] */);
/* Cosine instead of the dot product without the COO: installs weight = TKSPMV_ROW_INV_L2 as the engine's boost and removes any
 * installed bias -- the state tkspmv_set_boost(e, w, NULL) leaves, with w computed on the device (it never visits the host; every
 * entry is finite by construction, so nothing is checked). With a query of norm 1, tkspmv_run_boosted / tkspmv_enqueue_boosted with
 * both arrays NULL then return cosines. Like tkspmv_set_boost the call waits for the engine's stream first, allocates the weight
 * array on first use, and the boost counts as installed only once the launch has completed without error. Errors:
 * TKSPMV_ERR_INVALID for a NULL engine; TKSPMV_ERR_UNSUPPORTED where tkspmv_enqueue_row_stats reports it. */
int tkspmv_set_boost_cosine(tkspmv_t *e);
/* Assignment ("which of these vectors suits every row best?": nearest-centroid classification, the assignment step of spherical
 * k-means, routing rows to shards or topics, labelling a collection against prototype vectors), the opposite question to every query
 * form above. dev_xs holds count >= 1 dense vectors of desc.cols floats, back to back; every LOCAL row r (indexed like masks, group
 * labels and row statistics) receives
 *   best = s(r, 0); label = 0;  for q = 1 .. count-1: if (s(r, q) > best) { best = s(r, q); label = q; }
 *   dev_labels[r] = label (uint32), dev_best[r] = best (float32, optional)
 * with s(r, q) the fp32 score every other path reports for row r and vector q, bit for bit (tkspmv_scores, tkspmv_enqueue_score_rows,
 * the top-k lists): the sums are formed in the streaming kernels' order, and tkspmv_packed_assign restates them on the host. Ties go to
 * the smallest index. A row without entries scores +0.0f against every vector: label 0, best +0.0f. desc.min_score, the installed
 * filter, the installed query and the boost play no part. The vectors must be finite and yield scores that are not NaN; otherwise
 * the labels of the affected rows are unspecified. The labels are what tkspmv_set_groups, tkspmv_enqueue_facets (dev_labels) and
 * the masks of tkspmv_enqueue_col_stats are made from.
 * One pass over stream copy 0 of the matrix serves 16384 / T vectors held side by side in LDS, T the engine's column tier (1024,
 * 4096 or 16384 for up to that many columns): 16, 4 or 1 (assign_kernel); more vectors run as consecutive launches that merge with
 * the stored pair, behind a memset of both outputs on the same stream. dev_best = NULL is allowed only when count does not exceed the
 * vectors of one pass: the later launches keep their running scores in dev_best, and the engine owns no scratch that a call on a
 * caller's stream could use. Asynchronous, complete in stream order on any stream (NULL: the engine's); exactly desc.rows labels (and
 * scores) are written; reads and writes no engine state, so it may be mixed freely with the other calls, as tkspmv_enqueue_row_stats
 * may. With desc.rows = 0 the call succeeds and writes nothing.
 * Errors: TKSPMV_ERR_INVALID (checked first, before any device call) for a NULL engine, NULL dev_xs, NULL dev_labels or count < 1;
 * then TKSPMV_ERR_UNSUPPORTED exactly where tkspmv_enqueue_row_stats reports it (the approximate per-partition engines ARE served);
 * then TKSPMV_ERR_INVALID for dev_best = NULL with more vectors than one pass. A rejected call writes nothing. */
int tkspmv_enqueue_assign(tkspmv_t *e, const float *dev_xs, int32_t count, uint32_t *dev_labels /* [rows] */, float *dev_best /* [rows], may be NULL */,
                          void *stream);
/* The same with host arrays, any count with or without host_best: on engine-owned scratch (rows labels, rows scores, and the vectors
 * in chunks of at most 64 MiB), allocated by the first call, on the engine's stream; waits for its own launches only. */
int tkspmv_assign(tkspmv_t *e, const float *host_xs, int32_t count, uint32_t *host_labels /* [rows] */, float *host_best /* [rows], may be NULL */);
/* Nearest-n assignment ("which n of these vectors suit every row best, and by how much?": multi-assignment when an inverted-file
 * index is built, soft clustering, multi-label classification, the margin s1 - s2 of an assignment), optionally among the rows of an
 * allow-mask only (k-means on a subset, re-assigning one cluster's rows, classifying the rows a predicate lets through).
 * Inputs: count >= 1 dense vectors of desc.cols floats at dev_xs, back to back; 1 <= n <= TKSPMV_NEAREST_MAX_N; dev_mask, or NULL for
 * all rows: one bit per LOCAL row, LSB first, ceil(rows / 32) words, as in tkspmv_enqueue_filtered; bits at and beyond rows are
 * ignored.
 * Outputs: dev_labels[rows][n] (uint32) and dev_scores[rows][n] (float32), row-major: a row's list is contiguous.
 *  - A row is eligible if it is in the mask, or if there is no mask. Entry j of an eligible row r is the j-th of the vectors
 *    0 .. count-1 ordered by s(r, q) descending, then by index q ascending on a tie; scores compare as floats (-0.0 and +0.0 tie).
 *    s(r, q) is the fp32 score every other path reports for that row and vector, bit for bit (tkspmv_scores,
 *    tkspmv_enqueue_score_rows, the top-k lists, tkspmv_enqueue_assign); tkspmv_packed_nearest restates the lists on the host.
 *  - Entries j >= count are (TKSPMV_NEAREST_NONE, -inf).
 *  - An eligible row without entries scores +0.0f against every vector: labels 0, 1, .., scores +0.0f, then the padding.
 *  - A row outside the mask gets (TKSPMV_NEAREST_NONE, -inf) in every entry, so its labels fall into no bin of
 *    tkspmv_enqueue_label_sums or tkspmv_enqueue_facets.
 *  - n = 1 without a mask gives exactly the labels and bits of tkspmv_enqueue_assign.
 *  - desc.min_score, the installed query and filter and the boost play no part. NaN scores are outside the contract, as in assign.
 * One launch of nearest_fill_kernel writes every row's default list; then one pass over stream copy 0 of the matrix serves 16384 / T
 * vectors held in LDS (T the column tier: 16, 4 or 1 vectors, nearest_kernel), and more vectors run as consecutive launches that
 * merge with the stored list -- the running lists live in the outputs, so both are required. Asynchronous, complete in stream order
 * on any stream (NULL: the engine's); exactly rows * n words of each output are written; no engine state is read or written, so the
 * call may be mixed freely with the others. With desc.rows = 0 the call succeeds and writes nothing.
 * Errors: TKSPMV_ERR_INVALID (checked first, before any device call) for a NULL engine, dev_xs, dev_labels or dev_scores, count < 1
 * or n outside 1 .. TKSPMV_NEAREST_MAX_N; then TKSPMV_ERR_UNSUPPORTED exactly where tkspmv_enqueue_assign reports it and, with a
 * mask, where tkspmv_enqueue_col_stats with a mask does. A rejected call writes nothing. */
#define TKSPMV_NEAREST_MAX_N 4
#define TKSPMV_NEAREST_NONE 0xFFFFFFFFu
int tkspmv_enqueue_nearest(tkspmv_t *e, const float *dev_xs, int32_t count, int32_t n, const uint32_t *dev_mask /* NULL: all rows */,
                           uint32_t *dev_labels /* [rows][n] */, float *dev_scores /* [rows][n] */, void *stream);
/* The same with host arrays: on engine-owned scratch (rows * TKSPMV_NEAREST_MAX_N labels and scores, and the vectors in chunks of at
 * most 64 MiB, the vector index continuing across the chunks), allocated by the first call, on the engine's stream; waits for its
 * own launches only. use_filter != 0: among the rows of the installed allow-mask (tkspmv_set_filter); TKSPMV_ERR_STATE without one,
 * behind the checks above. */
int tkspmv_nearest(tkspmv_t *e, const float *host_xs, int32_t count, int32_t n, int32_t use_filter, uint32_t *host_labels /* [rows][n] */,
                   float *host_scores /* [rows][n], may be NULL */);
/* Label sums ("what does every cluster, class or topic look like?": the centroid update of (spherical) k-means -- the second half of
 * an iteration whose first half is tkspmv_enqueue_assign --, class prototypes for nearest-centroid classification, topic or shard
 * profiles; with one label the column sums of the matrix, or of a tkspmv_enqueue_match result turned into labels): np.add.at over the
 * COO keyed by (labels[row], col), without a COO and without leaving the device.
 * labels[r] (uint32, by LOCAL row, indexed like masks and group labels) names the bin of row r; a label >= n_bins has no bin, as in
 * tkspmv_enqueue_facets. dev_labels = NULL with n_bins = 0 takes the labels and the bin count installed by tkspmv_set_groups.
 *   sums[b][c] (int64, [n_bins][cols]) = the sum of quantise(v, E) over the COUNTED entries (r, c, v) with labels[r] == b
 * "Counted" is tkspmv_enqueue_col_stats' rule: every stored entry except the placeholder of an empty row and the padding behind a
 * partition's last row end; explicit zeros and a column repeated within a row each contribute.
 * quantise(v, E), E = quantum_exp, is integer arithmetic on the fp32 bit pattern (one function compiled for host and device):
 *   |v| = m * 2^x, m the 24-bit significand (a subnormal: no hidden bit, x = -149);  s = x - E;
 *   s >= 0: q = m << s;   s < 0: q = m >> -s, rounded to nearest with ties to even on the magnitude (a shift of 64 or more gives 0);
 *   the result takes the sign of v, so quantise(-v) = -quantise(v).
 * No floating-point instruction takes part. Defined for finite values with s <= 38; Inf, NaN and larger shifts leave the affected
 * words unspecified. The sums are integers added with integer atomics, so they are exact with respect to this rule and bit-identical
 * whatever the launch geometry, the partition cuts, the order of the atomics or the sharding: the int64 sums of the shards of a split
 * matrix, taken with ONE common E (the largest of the shards' tkspmv_sums_exponent), add up to the sums of the whole matrix -- an
 * integer all-reduce -- and tkspmv_enqueue_sums_close finishes the merged words. |ldexp(sums[b][c], E) - the exact sum| is at most
 * half a quantum per counted entry of the word.
 * mode: TKSPMV_SUMS_RAW writes dev_sums only; TKSPMV_SUMS_FLOAT and _UNIT add the closing launch into dev_out (float32,
 * [n_bins][cols], required):
 *   FLOAT  out[b][c] = ldexpf((float)sums[b][c], E), the int64 -> fp32 conversion rounding to nearest even; exactly n_bins * cols
 *          floats are written.
 *   UNIT   f_c = FLOAT's value; n2 = the sum over c of (double)f_c * (double)f_c, formed as 64 partials -- partial l takes the columns
 *          l, l + 64, ... ascending -- added in the order 0 .. 63; w = 1 / sqrt((float)n2) in two rounded fp32 operations, 0 where
 *          (float)n2 is 0 or not finite (tkspmv_enqueue_row_stats' TKSPMV_ROW_INV_L2 rule); out[b][c] = f_c * w. A bin with w == 0 --
 *          an empty cluster, a zero sum, an overflowed norm -- is NOT written: dev_out holding the previous centroids keeps them.
 * So tkspmv_enqueue_assign followed by tkspmv_enqueue_label_sums(UNIT, dev_out = the vectors of the next assign) is one iteration of
 * spherical k-means in stream order, with no host round trip.
 * flags: TKSPMV_SUMS_ACCUMULATE adds to what dev_sums holds instead of zeroing it in front (on the same stream): the shards of a
 * matrix, or its row blocks, into one buffer. TKSPMV_SUMS_SINK_LDS / _DIRECT force one of the kernel's two sinks -- bins in LDS
 * flushed per workgroup, 8192 / T bins per launch (T the column tier: 8 at 1024 columns, 2 at 4096, none at 16384), or one global
 * atomic per entry in one launch for any n_bins --, which the engine otherwise chooses by n_bins; the sums are the same bits
 * (label_sums_kernel). For tests and measurements.
 * Asynchronous, complete in stream order on any stream (NULL: the engine's); reads and writes no engine state, so it may be mixed
 * freely with the other calls. desc.min_score, the installed filter, the installed query and the boost play no part. With desc.rows =
 * 0 the call succeeds and leaves zeros. fp32 packet streams only.
 * Errors: TKSPMV_ERR_INVALID (checked first, before any device call) for a NULL engine, NULL or misaligned dev_sums, dev_labels
 * without n_bins or n_bins without dev_labels, n_bins > 2^30, an unknown mode or flag, both sink flags, or dev_out = NULL unless
 * RAW; then TKSPMV_ERR_UNSUPPORTED exactly where tkspmv_enqueue_row_stats reports it (the approximate per-partition engines and
 * engines made from a .tkspmv file ARE served); then TKSPMV_ERR_INVALID for dev_labels = NULL with no labels installed, or
 * TKSPMV_SUMS_SINK_LDS at the 16384-column tier. A rejected call writes nothing. */
#define TKSPMV_SUMS_RAW 0
#define TKSPMV_SUMS_FLOAT 1
#define TKSPMV_SUMS_UNIT 2
#define TKSPMV_SUMS_ACCUMULATE 1u
#define TKSPMV_SUMS_SINK_LDS 2u
#define TKSPMV_SUMS_SINK_DIRECT 4u
int tkspmv_enqueue_label_sums(tkspmv_t *e, const uint32_t *dev_labels /* [rows], may be NULL */, uint32_t n_bins, int32_t quantum_exp, uint32_t flags,
                              int64_t *dev_sums /* [n_bins][cols] */, int32_t mode, float *dev_out /* [n_bins][cols], may be NULL with RAW */, void *stream);
/* The closing launch alone (mode TKSPMV_SUMS_FLOAT or _UNIT, as above) over int64 sums the caller holds: merged shard sums, or sums
 * kept from a RAW call. Asynchronous, any stream, no engine state. TKSPMV_ERR_INVALID for a NULL engine, NULL or misaligned dev_sums,
 * NULL dev_out, n_bins outside 1 .. 2^30 or another mode. */
int tkspmv_enqueue_sums_close(tkspmv_t *e, const int64_t *dev_sums /* [n_bins][cols] */, uint32_t n_bins, int32_t quantum_exp, int32_t mode,
                              float *dev_out /* [n_bins][cols] */, void *stream);
/* The default exponent: E = xmax + 1 + ceil_log2(max(1, the fullest column's counted entries)) - 62, xmax the unbiased exponent of
 * the largest stored |v| (-126 for a subnormal or zero), from three tkspmv_col_stats passes (TKSPMV_COL_NNZ, _MAX, _MIN): with it no
 * sum can reach 2^63 whatever the labels, and at 1M x 1024 with 20 entries per row every value within 2^-13 of the largest is summed
 * exactly. A matrix without entries gives 0. A host form: waits. Shards whose sums are to be merged must use ONE common E: take the
 * maximum of theirs. Errors: TKSPMV_ERR_INVALID for a NULL argument; TKSPMV_ERR_UNSUPPORTED where tkspmv_col_stats reports it. */
int tkspmv_sums_exponent(tkspmv_t *e, int32_t *quantum_exp);
/* tkspmv_enqueue_label_sums with host arrays (host_labels = NULL with n_bins = 0: the installed labels): on engine-owned scratch
 * (rows labels, n_bins * cols sums and floats), allocated by the first call, on the engine's stream; waits for its own launches only.
 * Either output may be NULL (host_out only with RAW). With UNIT host_out is read first: a bin that is not written keeps its values. */
int tkspmv_label_sums(tkspmv_t *e, const uint32_t *host_labels /* [rows], may be NULL */, uint32_t n_bins, int32_t quantum_exp, int32_t mode,
                      int64_t *host_sums /* [n_bins][cols], may be NULL */, float *host_out /* [n_bins][cols], may be NULL with RAW */);
/* Column statistics ("how many rows carry this term, how large do its values get?": what IDF / BM25 query weights, score upper
 * bounds -- the sum over c of max(0, x[c] * max[c], x[c] * min[c]) bounds every row's score -- and significant-terms counts are made
 * of), taken from the matrix the engine already holds: np.bincount(col) without a COO, and in ONE pass what tkspmv_enqueue_match
 * answers with one pass per single-column predicate. One 4-byte word per column, desc.cols of them per SET; a set is all rows
 * (dev_mask = NULL, count must be 1) or the rows of one allow-mask (set i: dev_mask + i * mask_stride_words, indexed by LOCAL row like
 * every mask, ceil(rows / 32) words, bits at and beyond rows are ignored; stride 0: one mask for all sets). Set i's words are
 * written at dev_out + i * out_stride_words words (out_stride_words
 * >= cols when count > 1; the words between the sets are not touched):
 *   TKSPMV_COL_NNZ  uint32   the number of counted entries stored in column c; 0 for a column without one
 *   TKSPMV_COL_MAX  float32  the largest counted value; -inf for a column without a counted entry
 *   TKSPMV_COL_MIN  float32  the smallest counted value; +inf for a column without a counted entry
 * An entry is COUNTED when it is an entry of the COO as the packer stored it -- explicit zeros, negative values and a column repeated
 * within a row all count, the convention of TKSPMV_ROW_NNZ --, that is: not the placeholder of an empty row and not the padding behind
 * a partition's last row, and when its row is allowed by the set's mask, if the set has one.
 * Document frequency: COL_NNZ[c] equals the number of rows that carry column c -- the count tkspmv_enqueue_match reports for the
 * single-column clause {c} -- exactly when no row repeats column c; otherwise it is larger by the repeats.
 * Values compare in the engine's total order of scores (-0.0 < +0.0), so MAX / MIN are functions of the multiset of counted values;
 * NaNs compare wherever that order puts them. Integer add and max are associative and commutative: all three kinds are exact and
 * bit-reproducible whatever the launch geometry and the order of the atomics, and tkspmv_packed_col_stats restates them on the host.
 * desc.min_score, the installed query, the boost and the engine's result pair play no part. One pass over the matrix per set
 * (col_stats_kernel; up to 32 sets per launch, set i on stream copy i % stream_replicas; NNZ reads the column plane only) behind a
 * memset of the sets' words on the same stream, and for MAX / MIN one small closing launch. Asynchronous, complete in stream order on
 * any stream (NULL: the engine's); reads and writes no engine state, so it may be mixed freely with the other calls, as
 * tkspmv_enqueue_range may. Column SUMS are not offered: a float sum through atomics depends on their order.
 * Errors: TKSPMV_ERR_INVALID (checked first, before any device call) for a NULL engine, a NULL dev_out, a kind outside 0 .. 2,
 * count < 1, a NULL mask with count != 1, a negative stride, out_stride_words < cols with count > 1; TKSPMV_ERR_UNSUPPORTED where
 * tkspmv_enqueue_row_stats reports it (a packet stream that is not fp32), and with a mask where tkspmv_enqueue_filtered reports it
 * (the approximate per-partition engines are served without a mask only). */
#define TKSPMV_COL_NNZ 0
#define TKSPMV_COL_MAX 1
#define TKSPMV_COL_MIN 2
int tkspmv_enqueue_col_stats(tkspmv_t *e, int32_t kind, int32_t count, const uint32_t *dev_mask /* NULL: all rows, count must be 1 */,
                             int64_t mask_stride_words, void *dev_out /* [count] sets of cols words */, int64_t out_stride_words, void *stream);
/* One set into a host array of desc.cols words, on engine-owned scratch of that size (allocated by the first call), launched on the
 * engine's stream; waits for its own launch only. use_filter != 0: among the rows of the mask tkspmv_set_filter installed
 * (TKSPMV_ERR_STATE if none is installed). */
int tkspmv_col_stats(tkspmv_t *e, int32_t kind, int32_t use_filter, void *host_out /* [cols] */);
/* Several queries per pass over the matrix (an extension: the reference streams its matrix once per
 * query vector, host_spmv_bscsr.cpp:602-622). Same arguments and result contract as tkspmv_enqueue_batch. Needs
 * desc.multi_q != 0 at create time: info.multi_q queries share every chunk of the wave-sliced ELL copy of the matrix that
 * is loaded (x is held multi_q times in LDS; every query has its own accumulators, threshold, candidate lists and
 * exchange state). One lane owns one row and sums it in the row's own entry order, i.e. in the order of the reference's
 * gold (gold_algorithms.hpp:188-246): scores are bit-identical to the gold's sequential fp32 sums (tkspmv_run's differ
 * from those in the last bits: its sums follow the packet layout). Engines without the kernel (info.multi_q == 0:
 * desc.multi_q = 0, reduced precisions, more than 1024 columns, fewer publishing groups than k) run the ordinary
 * back-to-back sequence. dev_xs = NULL with count = 1: the vector installed by tkspmv_set_query.
 * At multi_q = 1 or 2 a launch makes several passes (8 / 4; option MULTI_PASSES), each over its own queries: invisible to the
 * caller, results and their order are the same. */
int tkspmv_enqueue_multi(tkspmv_t *e, const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream);
/* tkspmv_time_queries for the multi-query path: *ns_per_query = time of the whole sequence / iters. */
int tkspmv_time_multi(tkspmv_t *e, const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query);
/* Waits for the engine's stream. Results of queries enqueued with stream = NULL (the engine's own stream) are FINAL when this call
 * (or tkspmv_read, or any other engine call that waits for that stream) has returned: engines that stream with checked
 * workgroup-local thresholds (tkspmv_info.batch_mode bits 8-15) look at their launches' verdicts here and run a query whose check
 * failed again through the exact kernel -- the device-side equivalent of the reference's wait() after operator()
 * (host_spmv_bscsr.cpp:354-358). The query vectors of such launches must stay unchanged until then. (Option REPAIR=stream keeps the
 * exact launch behind every local launch in the stream, as it always is on a caller's stream: results are then final in stream
 * order, for 1-2 % of the time per query.) */
int tkspmv_synchronize(tkspmv_t *e);

/* Copy back the k results of the last completed query, sorted by (score desc, row desc)
 * (sort_tuples order, evaluation_utils.hpp:40-62). *n receives the count (always k; entries past the
 * number of qualifying rows are (0, 0.0f), as the gold's zero-initialised list). */
int tkspmv_read(tkspmv_t *e, uint32_t *idx, float *val, int32_t *n);
/* Device pointers of the engine-owned result buffers (k entries each). */
int tkspmv_result_device(tkspmv_t *e, const uint32_t **dev_idx, const float **dev_val);
/* Debug/verification: full score vector y = A.x of the current query (rows floats, host). */
int tkspmv_scores(tkspmv_t *e, float *host_y);

/* Diagnostics (TKSPMV_TRACE=1 at create time): per-wave 100 MHz wall-clock stamps of the last four launches,
 * [4][grid+1][9 waves][8] words: entry, x staged, first packet reduced, stream loop done, deferred packets judged,
 * flush done. tools/timeline.py turns them into a timeline. TKSPMV_ERR_STATE when tracing is off. */
int tkspmv_debug_trace(tkspmv_t *e, uint64_t *host, uint64_t max_words, uint64_t *words);
/* Diagnostics of the checked thresholds of back-to-back queries (tkspmv_info.batch_mode; no reference counterpart): out[0] =
 * selections whose check failed so far (each sent its query through the repair launch), out[1] = current suspension length of
 * carried thresholds (selections), out[2] = selections to go until they are used again, out[3] = batch launches so far, out[4] =
 * launches for which the workgroup-local thresholds as a whole stay switched off (a launch of which a quarter failed closes them
 * for 8 .. 1024 launches: data that keeps its best rows together), out[5] = the length of the latest such closure. n >= 6.
 * With n >= 10 also tkspmv_run's single-query kernel (workgroup-local thresholds, checked by its selection): out[6] = its
 * launches, out[7] = queries run again through the exact launch because the check failed, out[8] = failed checks as the device
 * counted them, out[9] = selections to go until carried thresholds are used again. With n >= 12: out[10] = batch launches that
 * went out without a repair launch behind them (see tkspmv_synchronize), out[11] = the late repairs that had to follow after all.
 * With n >= 14: out[12] = the pacing of back-to-back queries in force (pause quantum | levels << 8 | uniform pause << 16; units of
 * 128 cycles per packet), out[13] = microseconds tkspmv_create spent measuring it on this box (option AUTOTUNE; 0: static default).
 * With n >= 19 and option STATS, summed over the tkspmv_time_multi calls so far: out[14] = queries, out[15] = waves of the multi-query
 * kernel that ran into their bounded wait for a threshold, out[16] = the ticks (10 ns) spent there, out[17] / out[18] = rows offered
 * to / overflowed from the candidate lists.
 * Synchronises the engine's stream. */
int tkspmv_debug_counters(tkspmv_t *e, uint64_t *out, int32_t n);

/* `iters` queries back to back on the engine stream (cycling over n_x device-resident vectors), ONE hipEvent pair
 * around the batch: *ns_per_query = batch time / iters. Nothing else is launched (for profiler runs). */
int tkspmv_time_queries(tkspmv_t *e, const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query);
/* `reps` such batches back to back, all enqueued before the first wait, a hipEvent between consecutive ones: ns_per_query[r] =
 * time of batch r / iters. The GPU does not idle between batches (a batch that follows a host-side gap runs 10-25 % slower for
 * about a millisecond: power management), so median and p95 of these are the kernel's under sustained load. reps <= 4096. */
int tkspmv_time_query_batches(tkspmv_t *e, const float *dev_xs, int32_t n_x, int32_t iters, int32_t reps, double *ns_per_query);
/* Measurement aid: the reference's loop -- reset(x) from host memory, operator(), read_result(): host_spmv_bscsr.cpp:602-632 --
 * run `iters` times in native code over n_x host vectors (stride cols floats): loop_ns[i] = the host's steady clock around
 * tkspmv_set_query + tkspmv_run + tkspmv_read of iteration i (what the reference reports as hw_full_exec_time + its reset),
 * kernel_ns[i] (may be NULL) = tkspmv_run's own figure. A caller that goes through a foreign-function layer pays that layer's
 * transitions on top (three per iteration). */
int tkspmv_time_host_loop(tkspmv_t *e, const float *host_xs, int32_t n_x, int32_t iters, double *loop_ns, double *kernel_ns);
/* Measurement aid: `passes` passes over the engine's packet stream (rotating its stream copies) by a kernel with the
 * engine's launch geometry that only LOADS the packets -- no x, no arithmetic, no selection -- in ONE launch, inside one
 * hipEvent pair: *ns_per_pass = what moving the stream from HBM into registers costs on this GPU. bench.py prints the
 * streaming kernels' time against it next to the fraction of the 8 TB/s specification. */
int tkspmv_time_stream_read(tkspmv_t *e, int32_t passes, double *ns_per_pass);

/* Benchmark helper: run `iters` queries cycling over `n_x` device-resident vectors (stride cols floats)
 * back-to-back on the engine stream, timed with hipEvents on that stream. */
int tkspmv_profile(tkspmv_t *e, const float *dev_xs, int32_t n_x, int32_t iters, tkspmv_timing *out);

/* Engine options (no reference counterpart: the reference fixes its variants at compile time, types.hpp / the Makefile's -D flags).
 * Every switch that changes what an engine does is one row of a documented table (csrc/options.cpp; tkspmv_option_info lists it at
 * run time: `bin/approximate-spmv-mi355x-topk --options` prints it): threshold scheme, batching, layouts, host hand-off, multi-GPU
 * merge, diagnostics. An option is read when an engine, a packed matrix or a communicator is CREATED; tkspmv_set_option(name, value)
 * sets it for the creations that follow in this process (value NULL: back to unset = the engine's own default), and the
 * environment variable TKSPMV_<NAME> is the same option for shell-driven runs (a value set through this call wins).
 * Returns TKSPMV_ERR_INVALID for a name that is not in the table. tkspmv_get_option: the current value or NULL.
 * tkspmv_option_info(i, ...): row i of the table (0 <= i < tkspmv_option_count()); any out pointer may be NULL. */
int tkspmv_set_option(const char *name, const char *value);
const char *tkspmv_get_option(const char *name);
int tkspmv_option_count(void);
int tkspmv_option_info(int32_t i, const char **name, const char **kind, const char **values, const char **doc);

const char *tkspmv_last_error(void);
int tkspmv_device_count(void);

/* ---- row-sharded multi-GPU step (one process per GPU) ---------------------------------------------------------
 * The reference merges its row partitions on the host (src/fpga/src/host_spmv_bscsr.cpp:399-448, global id =
 * local + first_row at :415). One level up: every rank owns an engine over its row shard (desc.first_row = first
 * global row), per query the local fused kernel, ONE RCCL all-gather of k (row, score) pairs per rank and a merge
 * kernel. Queries are exchanged in batches (default 32, TKSPMV_DIST_BATCH / tkspmv_dist_set_batch; 1 = every query on
 * its own): the local step of a batch is launched as one back-to-back sequence when the batch closes (passes of several
 * queries each if the engine was created with desc.multi_q), then one
 * all-gather and one merge launch per batch on a side stream, overlapping the local step of the next batch (two buffer
 * sets). synchronize / read flush an open batch; a query vector passed to tkspmv_dist_enqueue must stay valid until then. Every rank must issue the same call sequence. RCCL is
 * loaded with dlopen inside tkspmv_dist_create / tkspmv_dist_unique_id: TKSPMV_ERR_UNSUPPORTED if it cannot be loaded.
 *
 * What the merge computes (tkspmv_dist_read*, tkspmv_merge_topk*, and distributed.merge_candidates in the Python package):
 *   - A shard list is k entries in tkspmv_read order: real entries first, then fillers (row 0, score bits 0x00000000).
 *   - The FILLER SUFFIX of a list is its maximal suffix of entries with row id 0 and score bits exactly 0x00000000.
 *     (0, -0.0f) (bits 0x80000000) is a real entry, and so is (r > 0, +0.0f).
 *   - The merged list is all real entries of all shards, sorted by (order key of the score descending, row id descending as
 *     unsigned 32-bit), cut at k; if there are fewer than k, the tail is padded with (0, 0.0f). A filler never outranks a real
 *     entry, for any desc.min_score (with min_score < 0 real scores are negative, and +0.0f would sort above them).
 *   - One case cannot be told apart: on the shard with first_row = 0, a real LAST entry "row 0 scoring +0.0f" is
 *     indistinguishable from a filler and is treated as one. This changes the output only when min_score < 0 (otherwise it
 *     would sort last among the real entries anyway, and the padding restores it). With world = 1 the merged list is the
 *     engine's own list.
 *   - Non-finite scores have no stated contract here.
 *   - Limit: world * k <= 8184 (the merge block keeps world * k 64-bit keys and 8 padding keys in its 64 KiB of LDS), so
 *     world = 8 with k = 1024 is refused (k <= 1023 at world 8): TKSPMV_ERR_INVALID from tkspmv_dist_create and tkspmv_merge_topk*. */
typedef struct tkspmv_dist tkspmv_dist_t;
/* rank 0 creates the 128-byte RCCL unique id and ships it to the other ranks (any transport). */
int tkspmv_dist_unique_id(uint8_t *out128);
/* id128 may be NULL when world == 1. The engine must outlive the returned object. world * k <= 8184 (k: the engine's). */
int tkspmv_dist_create(tkspmv_dist_t **out, tkspmv_t *engine, const uint8_t *id128, int32_t rank, int32_t world);
int tkspmv_dist_set_batch(tkspmv_dist_t *d, int32_t batch);                    /* 1..32 queries per exchange */
int tkspmv_dist_enqueue(tkspmv_dist_t *d, const float *dev_x);                 /* one query, asynchronous */
int tkspmv_dist_run_many(tkspmv_dist_t *d, const float *dev_xs, int32_t n_x, int32_t count);
int tkspmv_dist_synchronize(tkspmv_dist_t *d);
/* merged (global) top-k of the most recently enqueued query (host buffers of k entries); waits for it */
int tkspmv_dist_read(tkspmv_dist_t *d, uint32_t *idx, float *val, int32_t *n);
/* The exchange step alone, for measurement (collective: every rank calls it with the same arguments): `iters` times the
 * all-gather of one full batch (batch x 2k words per rank) + the merge launch, back to back on the communication stream,
 * one hipEvent pair around them. */
int tkspmv_dist_read_batch(tkspmv_dist_t *d, uint32_t *idx, float *val, int32_t *n_q);  /* every list of the last exchanged batch: [n_q][k] */
int tkspmv_dist_time_exchange(tkspmv_dist_t *d, int32_t iters, double *ns_per_exchange);
void tkspmv_dist_destroy(tkspmv_dist_t *d);
const char *tkspmv_dist_last_error(void);
/* The merge of an exchange batch as the pipelined step launches it: dev_gathered [world][n_q][2][k] u32 (row ids, then score
 * bits), one block per query, results [n_q][k] (1 <= n_q <= 32): exactly n_q * k entries of dev_idx and of dev_val are written.
 * Lifts the host-side merge of host_spmv_bscsr.cpp:399-448 for a batch of queries. The lists and the result follow the contract
 * stated above (filler suffix, order, padding); world >= 1, k >= 1 and world * k <= 8184, else TKSPMV_ERR_INVALID and nothing
 * is launched. */
int tkspmv_merge_topk_batch(const uint32_t *dev_gathered, int32_t world, int32_t n_q, int32_t k, uint32_t *dev_idx,
                            float *dev_val, void *stream);
/* Rehearsal without RCCL (which refuses two ranks on one device): the all-gather of the pipelined step goes through host
 * buffers and this callback (send: this rank's bytes_per_rank bytes; recv: world such blocks, rank-major; 0 = success);
 * everything else -- batches, buffer rotation, events, merge launch -- is the real step. With TKSPMV_DIST_NO_NCCL=1
 * tkspmv_dist_create builds no communicator for world > 1 and the callback is mandatory. */
typedef int (*tkspmv_host_allgather_fn)(const void *send, void *recv, uint64_t bytes_per_rank, void *user);
int tkspmv_dist_set_host_exchange(tkspmv_dist_t *d, tkspmv_host_allgather_fn fn, void *user);
/* The merge step alone, one query: dev_gathered = [world][2][k] u32 -> the k best in dev_idx / dev_val [k]. Same contract and
 * the same limit (world * k <= 8184) as tkspmv_merge_topk_batch with n_q = 1. */
int tkspmv_merge_topk(const uint32_t *dev_gathered, int32_t world, int32_t k, uint32_t *dev_idx, float *dev_val,
                      void *stream);

/* ---- host-side helpers (no GPU needed) --------------------------------------------------------- */
typedef struct {
    uint32_t rows, cols;   /* from the size line */
    uint64_t nnz;
    uint32_t *row, *col;   /* malloc'd, release with tkspmv_mtx_free */
    float *val;
    uint32_t num_rows_coo; /* max(row)+1, as coo_t derives it (coo_matrix.hpp:21-27) */
    int32_t index_base;    /* index base actually applied: 0 or 1 */
    int32_t symmetric;     /* banner said symmetric */
} tkspmv_coo;

/* index_base: 0 = file is zero-indexed (the reference's compiled-in behaviour, zero_indexed_file=true),
 *             1 = file is one-indexed (create_matrices.py output), -1 = auto-detect (min index == 0 ? 0 : 1).
 * read_values = 0 => all values 1.0 (reference -v). sort = non-zero => (row,col) sort like customSort. */
int tkspmv_mtx_read(const char *path, int32_t index_base, int32_t read_values, int32_t sort, tkspmv_coo *out);
void tkspmv_mtx_free(tkspmv_coo *m);
int tkspmv_mtx_write(const char *path, uint32_t rows, uint32_t cols, uint64_t nnz, const uint32_t *row,
                     const uint32_t *col, const float *val, int32_t index_base, int32_t precision);

/* create_sample_vector(vec,size,random,sum_to_one,norm_one,seed): seed==0 => std::random_device. */
int tkspmv_sample_vector(float *vec, int32_t size, int32_t random, int32_t sum_to_one, int32_t norm_one, int32_t seed);

/* Synthetic matrix with the distributions of create_matrices.py (dist: 0 = uniform, 1 = gamma). Own PRNG. */
int tkspmv_generate(uint32_t rows, uint32_t cols, uint32_t avg_nnz, int32_t dist, uint64_t seed, tkspmv_coo *out);
/* Rows [row_begin, row_end) of that matrix with LOCAL row ids (row - row_begin): every row has its own PRNG streams, so a
 * slice equals the corresponding rows of the whole matrix -- what one rank of a row-sharded job builds (BASELINE configs[3]:
 * 10M rows over 8 GPUs; the 10M-row COO never exists in one process). tkspmv_generate_degrees: the row lengths alone
 * (deg[row_end - row_begin]), from which nnz-balanced shard bounds are computed without generating any entry. */
int tkspmv_generate_rows(uint32_t row_begin, uint32_t row_end, uint32_t cols, uint32_t avg_nnz, int32_t dist, uint64_t seed,
                         tkspmv_coo *out);
int tkspmv_generate_degrees(uint32_t row_begin, uint32_t row_end, uint32_t avg_nnz, int32_t dist, uint64_t seed,
                            uint32_t *deg);

typedef struct {
    char matrix_path[1024];
    int32_t use_sample_matrix, reset, num_tests, debug, ignore_matrix_values, top_k_value;
    char xclbin_path[1024];
    int32_t gpu_impl, use_half_precision_gpu, block_size_1d, block_size_2d, num_blocks;
} tkspmv_options;
int tkspmv_options_parse(int argc, char **argv, tkspmv_options *out);

/* Layout introspection for tests: pack on the host, decode back to COO (+ placeholders dropped). */
typedef struct tkspmv_packed tkspmv_packed;
int tkspmv_pack(const tkspmv_desc *desc, uint32_t n_wave_partitions_hint, tkspmv_packed **out);
int tkspmv_packed_info(const tkspmv_packed *p, tkspmv_info *info);
/* Decodes into caller arrays sized >= nnz; returns the number of decoded entries in *n. */
int tkspmv_packed_decode(const tkspmv_packed *p, uint32_t *row, uint32_t *col, float *val, uint64_t *n);
/* Raw views (host memory owned by p). */
int tkspmv_packed_raw(const tkspmv_packed *p, const void **packets, uint64_t *packet_bytes, const uint32_t **pkt_row,
                      const uint32_t **part_first, const uint32_t **part_count, uint32_t *n_parts);
/* One row of a packed matrix: its entries in stream order (= the order of the COO). *n = the row's length, also beyond
 * capacity; min(*n, capacity) entries are written (col / val may be NULL with capacity = 0). Found by bisecting the packets' row
 * table (csrc/row_lookup.hpp, the lookup the engine's row_vectors_kernel runs), not by decoding the stream. No GPU needed.
 * TKSPMV_ERR_INVALID for row >= rows, TKSPMV_ERR_UNSUPPORTED for value types other than TKSPMV_F32. */
int tkspmv_packed_get_row(const tkspmv_packed *p, uint32_t row, uint32_t *col, float *val, uint32_t capacity, uint32_t *n);
/* Scores of rows of a packed matrix for one vector x of cols floats: scores[i] = the fp32 score of LOCAL row rows[i], with the bits
 * an engine created from this packed matrix reports for it (tkspmv_enqueue_score_rows, tkspmv_scores): the row is looked up as
 * tkspmv_packed_get_row looks it up and its own packets go through the streaming kernels' arithmetic, restated for the host. A row
 * without entries scores +0.0f. No GPU needed. TKSPMV_ERR_INVALID for a NULL argument, n_rows < 1 or a row >= rows (nothing is
 * written then), TKSPMV_ERR_UNSUPPORTED for value types other than TKSPMV_F32. */
int tkspmv_packed_score_rows(const tkspmv_packed *p, const float *x, const uint32_t *rows, int32_t n_rows, float *scores);
/* One statistic (TKSPMV_ROW_NNZ .. TKSPMV_ROW_INV_L2) of EVERY row of a packed matrix: out[r], rows floats, with the bits an engine
 * created from this packed matrix reports (tkspmv_enqueue_row_stats): the lookup and the restated arithmetic of
 * tkspmv_packed_score_rows, with each product replaced by 1, |v| or v * v. No GPU needed. TKSPMV_ERR_INVALID for a NULL argument or
 * a kind outside 0 .. 3, TKSPMV_ERR_UNSUPPORTED for value types other than TKSPMV_F32; a rejected call writes nothing. */
int tkspmv_packed_row_stats(const tkspmv_packed *p, int32_t kind, float *out /* [rows] */);
/* Label and best score of EVERY row of a packed matrix against count vectors of cols floats (xs, back to back): labels[r] and best[r],
 * rows of each, with the bits an engine created from this packed matrix reports (tkspmv_enqueue_assign): every row's
 * tkspmv_packed_score_rows score against each vector in turn, the first kept and a later one only where it is strictly greater. A
 * row without entries gets label 0 and +0.0f. No GPU needed. TKSPMV_ERR_INVALID for a NULL matrix, NULL xs, NULL labels or
 * count < 1, TKSPMV_ERR_UNSUPPORTED for value types other than TKSPMV_F32; a rejected call writes nothing. */
int tkspmv_packed_assign(const tkspmv_packed *p, const float *xs, int32_t count, uint32_t *labels /* [rows] */, float *best /* [rows], may be NULL */);
/* The n best of count vectors for EVERY row of a packed matrix, in order: labels[rows][n] and scores[rows][n] with the bits an engine
 * created from this packed matrix reports (tkspmv_enqueue_nearest, whose contract this restates): every eligible row's
 * tkspmv_packed_score_rows score against each vector in turn, each placed behind the entries that score at least as much. mask: one
 * bit per row, ceil(rows / 32) words, or NULL for all rows. No GPU needed. TKSPMV_ERR_INVALID for a NULL matrix, xs, labels or scores,
 * count < 1 or n outside 1 .. TKSPMV_NEAREST_MAX_N, TKSPMV_ERR_UNSUPPORTED for value types other than TKSPMV_F32; a rejected call
 * writes nothing. */
int tkspmv_packed_nearest(const tkspmv_packed *p, const float *xs, int32_t count, int32_t n, const uint32_t *mask /* may be NULL */,
                          uint32_t *labels /* [rows][n] */, float *scores /* [rows][n] */);
/* The label sums of a packed matrix (tkspmv_enqueue_label_sums' contract, with the bits an engine created from this packed matrix
 * reports): every row located in the stream and its entries' quantise(v, E) added to sums[labels[r]][c], then the closing rule of
 * `mode` into out (UNIT: a bin whose w is 0 is not written and keeps what out holds). sums may be NULL; out only with
 * TKSPMV_SUMS_RAW. No GPU needed. TKSPMV_ERR_INVALID for a NULL matrix, NULL labels, n_bins outside 1 .. 2^30, an unknown mode or
 * out = NULL unless RAW; TKSPMV_ERR_UNSUPPORTED for value types other than TKSPMV_F32; a rejected call writes nothing. */
int tkspmv_packed_label_sums(const tkspmv_packed *p, const uint32_t *labels /* [rows] */, uint32_t n_bins, int32_t quantum_exp, int32_t mode,
                             int64_t *sums /* [n_bins][cols], may be NULL */, float *out /* [n_bins][cols], may be NULL with RAW */);
/* tkspmv_sums_exponent of a packed matrix, from tkspmv_packed_col_stats' three statistics. The closing rule alone over int64 sums
 * (tkspmv_enqueue_sums_close on the host; UNIT: see above) is tkspmv_packed_label_sums' second half and needs no matrix: cols is given. */
int tkspmv_packed_sums_exponent(const tkspmv_packed *p, int32_t *quantum_exp);
int tkspmv_sums_close_host(const int64_t *sums /* [n_bins][cols] */, uint32_t n_bins, uint32_t cols, int32_t quantum_exp, int32_t mode, float *out /* [n_bins][cols] */);
/* quantise(v, E) of the value with the fp32 bit pattern value_bits: the function the kernel and the host twin share. */
int64_t tkspmv_quantise(uint32_t value_bits, int32_t quantum_exp);
/* One column statistic (TKSPMV_COL_NNZ .. TKSPMV_COL_MIN) of a packed matrix over all rows (mask = NULL) or the rows of an allow-mask
 * of ceil(rows / 32) words: out[c], cols words, with the bits an engine created from this packed matrix reports
 * (tkspmv_enqueue_col_stats): a plain walk over the packet stream, so it works on a loaded .tkspmv file with no COO. No GPU needed.
 * TKSPMV_ERR_INVALID for a NULL matrix or output or a kind outside 0 .. 2, TKSPMV_ERR_UNSUPPORTED for value types other than
 * TKSPMV_F32; a rejected call writes nothing. */
int tkspmv_packed_col_stats(const tkspmv_packed *p, int32_t kind, const uint32_t *mask /* NULL: all rows */, void *out /* [cols] */);
void tkspmv_packed_free(tkspmv_packed *p);
/* The DEVICE packer (what tkspmv_create uses by default): packs desc's COO with HIP kernels on desc->device
 * and copies the result back into a tkspmv_packed, so that it can be compared byte for byte with tkspmv_pack's
 * (tkspmv_packed_raw) or saved. ms[0] = upload of the COO, ms[1] = packing kernels (ms may be NULL). Needs a GPU. */
int tkspmv_pack_device(const tkspmv_desc *desc, uint32_t n_wave_partitions_hint, tkspmv_packed **out, double *ms);
/* The same for the wave-sliced ELL layout of the multi-query kernel (wsell.hpp): packs desc's COO for
 * n_wave_partitions_hint waves and decodes it again into caller arrays sized >= nnz (entries grouped by row, rows in
 * stream order). info[0..5] = slices, chunks, padded entries, partitions, stream bytes, most chunks in one partition. */
int tkspmv_sell_roundtrip(const tkspmv_desc *desc, uint32_t n_wave_partitions_hint, uint32_t *row, uint32_t *col, float *val,
                          uint64_t *n, uint64_t *info);
/* Packs desc's COO into that layout twice -- on the host and with the device packer tkspmv_create uses (plan on the
 * host, fill kernel on desc->device) -- and compares the two byte for byte, side tables included.
 * info[0] = 1 if identical, info[1] = stream bytes, info[2] = chunks; ms[0] = host packer, ms[1..3] = device packer:
 * plan, uploads (the COO included), fill kernel (ms may be NULL). Needs a GPU. */
int tkspmv_sell_pack_device_check(const tkspmv_desc *desc, uint32_t n_wave_partitions_hint, uint64_t *info, double *ms);

/* ---- packed-matrix cache ------------------------------------------------------------------------
 * The reference parses the MatrixMarket text (utils.hpp:380-388, minutes at 10^7 rows) and packs
 * (host_spmv_bscsr.cpp:133-248, `hw_setup_time_ms`) on every run. Here the packed matrix can be written once
 * (".tkspmv": 128-byte header, packet stream, side tables, checksum) and an engine created straight from it.
 * tkspmv_wave_partitions: how many streaming waves a launch on desc->device has (pass it to tkspmv_pack as the hint
 * so that the file suits that GPU; a file with MORE partitions is rejected with TKSPMV_ERR_UNSUPPORTED unless the engine
 * deals the partitions out dynamically -- fp32 values, at most 1024 columns: tkspmv_info.claim_sets -- where any count
 * works and tkspmv_create itself cuts ~2 sets of 8 per workgroup; fewer is fine everywhere). tkspmv_packed_load: TKSPMV_ERR_IO for a missing, truncated,
 * inconsistent or corrupted file. tkspmv_create_packed: rows/cols/nnz and the value type come from the packed matrix,
 * everything else (k, device, min_score, first_row, stream_replicas, TKSPMV_Q1_7 vs TKSPMV_Q1_7_WIDE) from desc. */
int tkspmv_wave_partitions(const tkspmv_desc *desc, uint32_t *n);
int tkspmv_packed_save(const tkspmv_packed *p, const char *path);
int tkspmv_packed_load(const char *path, tkspmv_packed **out);
int tkspmv_create_packed(tkspmv_t **out, const tkspmv_packed *p, const tkspmv_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TKSPMV_H */
