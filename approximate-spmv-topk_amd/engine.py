"""Python mirror of the reference's engine concept `struct SpMV` (setup in the constructor, then per query
reset(vec) -> operator()() -> read_result()), bound to the HIP engine through the C ABI (include/tkspmv.h).

  SpMV(...)            <- src/gpu/host_spmv_topk_csr_gpu.cu:95-169, src/fpga/src/host_spmv_bscsr.cpp:104-131
  SpMV.__call__(debug) <- operator()(int debug): runs one query, returns the kernel time in ns  (:171 / :323)
  SpMV.read_result()   <- read_result(res, res_idx): (values, indices), value-descending       (:233 / :399)
  SpMV.reset(vec)      <- reset(vec, debug): installs a new query vector, returns ns          (:241 / :450)

The compute path is the HIP library only; constructing an engine without a GPU raises TkspmvError(ERR_DEVICE).
"""
import ctypes as C
from contextlib import contextmanager

import numpy as np

from . import _lib
from ._lib import f32p, ptr, u32p
from .host import _allow_words, _vectors

MAX_PAGE = 1000  # ranked_spmv's default page: every page takes the scores + radix-select route whatever k is, so a large page is cheapest


class SpMV:
    _n_groups = 0  # bins of the labels installed by set_groups (0: none); run_facets sizes its host arrays by it

    def __init__(self, x, y, val, num_rows, num_cols, num_nnz=None, vec=None, k=20, debug=0, *, device=-1,
                 first_row=0, min_score=0.0, partitions=1, k_per_partition=0, precision=_lib.F32, waves_per_cu=0,
                 threads_per_wg=0, nnz_per_lane=0, stream_replicas=0, fixed_width=0, multi_q=0, impl=0):
        """x, y, val: row-sorted COO (row ids, column ids, values) as the FPGA host passes them
        (host_spmv_bscsr.cpp:585); val=None means all ones (-v). precision=FIXED: the FPGA's fixed-point real_type of
        `fixed_width` bits (8..32; 0 = 32, the reference's FIXED_WIDTH default, types.hpp:20)."""
        self._h = C.c_void_p()
        row = np.ascontiguousarray(x, dtype=np.uint32)
        col = np.ascontiguousarray(y, dtype=np.uint32)
        v = None if val is None else np.ascontiguousarray(val, dtype=np.float32)
        nnz = int(row.shape[0]) if num_nnz is None else int(num_nnz)
        d = _lib.Desc()
        d.rows, d.cols, d.nnz = int(num_rows), int(num_cols), nnz
        d.row, d.col, d.val = u32p(row), u32p(col), f32p(v)
        d.k, d.partitions, d.k_per_partition, d.precision = int(k), int(partitions), int(k_per_partition), precision
        d.device, d.first_row, d.min_score = int(device), int(first_row), float(min_score)
        d.waves_per_cu, d.threads_per_wg, d.nnz_per_lane = int(waves_per_cu), int(threads_per_wg), int(nnz_per_lane)
        d.stream_replicas = int(stream_replicas)
        d.fixed_width = int(fixed_width)
        d.multi_q = int(multi_q)
        d.impl = int(impl)
        _lib.check(_lib.lib().tkspmv_create(C.byref(self._h), C.byref(d)))
        self._created(k, int(num_rows), int(num_cols), nnz, first_row, debug, vec)

    def _created(self, k, num_rows, num_cols, num_nnz, first_row, debug, vec):
        """What __init__ and from_packed share once the handle exists: the engine's sizes as attributes, then the first vector."""
        self.k = int(k)
        self.num_rows, self.num_cols, self.num_nnz = num_rows, num_cols, num_nnz
        self.first_row = int(first_row)
        self.debug = debug
        if vec is not None:
            self.reset(vec)

    @classmethod
    def from_packed(cls, packed, k=20, debug=0, *, vec=None, device=-1, first_row=0, min_score=0.0, precision=None,
                    stream_replicas=0, multi_q=0):
        """Engine straight from a packed matrix (host.Packed, e.g. Packed.load("matrix.tkspmv")): no MatrixMarket
        parsing, no packing. precision: None = the packed value type (F32 / Q1_7 / F16 / FIXED), or Q1_7_WIDE for Q1.7 values."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        info = packed.info()
        d = _lib.Desc()
        d.rows, d.cols, d.nnz = info["rows"], info["cols"], info["nnz"]
        d.k = int(k)
        d.precision = info["precision"] if precision is None else precision
        d.device, d.first_row, d.min_score = int(device), int(first_row), float(min_score)
        d.stream_replicas = int(stream_replicas)
        d.multi_q = int(multi_q)
        _lib.check(_lib.lib().tkspmv_create_packed(C.byref(self._h), packed._h, C.byref(d)))
        self._created(k, info["rows"], info["cols"], info["nnz"], first_row, debug, vec)
        return self

    # -- the four verbs ---------------------------------------------------------------------------------
    def reset(self, vec, debug=0):
        v = np.ascontiguousarray(vec, dtype=np.float32)
        if v.shape[0] != self.num_cols:
            raise ValueError(f"query vector has {v.shape[0]} entries, expected {self.num_cols}")
        ns = C.c_double()
        _lib.check(_lib.lib().tkspmv_set_query(self._h, f32p(v), C.byref(ns)))
        return int(ns.value)

    def __call__(self, debug=0):
        ns = C.c_double()
        _lib.check(_lib.lib().tkspmv_run(self._h, C.byref(ns)))
        return ns.value

    def read_result(self, debug=0):
        idx = np.empty(self.k, dtype=np.uint32)
        val = np.empty(self.k, dtype=np.float32)
        n = C.c_int32()
        _lib.check(_lib.lib().tkspmv_read(self._h, u32p(idx), f32p(val), C.byref(n)))
        return val[:n.value], idx[:n.value]

    # -- extras -----------------------------------------------------------------------------------------
    def reset_device(self, dev_ptr):
        """Query vector already resident in HBM (raw device pointer, e.g. torch tensor.data_ptr())."""
        _lib.check(_lib.lib().tkspmv_set_query_device(self._h, ptr(dev_ptr)))

    def enqueue(self, dev_x=0, dev_idx=0, dev_val=0, stream=0):
        """Asynchronous launch of one query on `stream` (raw hipStream_t handle; 0 = engine stream)."""
        _lib.check(_lib.lib().tkspmv_enqueue(self._h, ptr(dev_x), ptr(dev_idx), ptr(dev_val), ptr(stream)))

    def enqueue_many(self, dev_xs, n_x, count, stream=0):
        """`count` queries back to back from a device array of n_x query vectors (no host sync)."""
        _lib.check(_lib.lib().tkspmv_enqueue_many(self._h, ptr(dev_xs), int(n_x), int(count), ptr(stream)))

    def time_queries(self, dev_xs, n_x, iters):
        """ns per query of `iters` back-to-back queries (one hipEvent pair around the batch; nothing else launched)."""
        ns = C.c_double()
        _lib.check(_lib.lib().tkspmv_time_queries(self._h, ptr(dev_xs), int(n_x), int(iters), C.byref(ns)))
        return ns.value

    def time_host_loop(self, host_xs, iters):
        """The reference's reset / operator() / read_result loop run natively `iters` times over the rows of host_xs (float32,
        [n_x, cols]): (loop_us[iters], kernel_us[iters]) -- the host clock around the three calls, and tkspmv_run's own figure."""
        xs = np.ascontiguousarray(host_xs, dtype=np.float32)
        loop, kern = (C.c_double * int(iters))(), (C.c_double * int(iters))()
        _lib.check(_lib.lib().tkspmv_time_host_loop(self._h, f32p(xs), int(xs.shape[0]), int(iters), loop, kern))
        return np.array(loop, dtype=np.float64) / 1e3, np.array(kern, dtype=np.float64) / 1e3

    def time_query_batches(self, dev_xs, n_x, iters, reps):
        """`reps` batches of `iters` back-to-back queries, all enqueued before the first wait: ns per query of every batch (the GPU
        never idles between them: the kernel under sustained load)."""
        out = (C.c_double * int(reps))()
        _lib.check(_lib.lib().tkspmv_time_query_batches(self._h, ptr(dev_xs), int(n_x), int(iters), int(reps), out))
        return [float(v) for v in out]

    def time_stream_read(self, passes):
        """ns per pass of a kernel that only loads the engine's packet stream (engine geometry, one launch, rotating
        stream copies): the floor this GPU sets for any kernel that streams the matrix (measurement aid)."""
        ns = C.c_double()
        _lib.check(_lib.lib().tkspmv_time_stream_read(self._h, int(passes), C.byref(ns)))
        return ns.value

    def enqueue_batch(self, dev_xs, count, dev_idx=0, dev_val=0, stream=0):
        """A batch of `count` queries (rows of a device array, stride cols floats); query i's k results go to
        dev_idx + i*k / dev_val + i*k (device pointers; 0 => engine buffers, last query wins). No host sync."""
        _lib.check(_lib.lib().tkspmv_enqueue_batch(self._h, ptr(dev_xs), int(count), ptr(dev_idx), ptr(dev_val), ptr(stream)))

    def enqueue_filtered(self, dev_xs, count, dev_mask, mask_stride=0, dev_idx=0, dev_val=0, stream=0):
        """Filtered top-k of `count` queries: query i (dev_xs + i*cols; dev_xs = 0 with count = 1: the vector installed by reset())
        restricted to the rows set in the allow-mask dev_mask + i*mask_stride words (mask_stride = 0: one mask for every query;
        dev_mask = 0: the mask installed by set_filter). Masks are uint32 words as row_mask() builds them. Results as in
        enqueue_batch. No host sync."""
        _lib.check(_lib.lib().tkspmv_enqueue_filtered(self._h, ptr(dev_xs), int(count), ptr(dev_mask), int(mask_stride), ptr(dev_idx), ptr(dev_val),
                                                      ptr(stream)))

    def set_filter(self, mask_words):
        """Installs an allow-mask (row_mask() words, ceil(rows/32) of them) for enqueue_filtered(dev_mask=0); None removes it."""
        if mask_words is None:
            _lib.check(_lib.lib().tkspmv_set_filter(self._h, None))
            return
        w = np.ascontiguousarray(mask_words, dtype=np.uint32)
        if w.shape != ((self.num_rows + 31) // 32,):
            raise ValueError(f"allow-mask has {w.size} words, expected {(self.num_rows + 31) // 32} for {self.num_rows} rows")
        _lib.check(_lib.lib().tkspmv_set_filter(self._h, u32p(w)))

    def _install(self, vec=None, allow=None, groups=None):
        """The prologue of the host-array query forms, each step only if its argument is given: reset(vec), then set_filter(allow)
        (a bool array of length rows, or row_mask() words), then set_groups(groups)."""
        if vec is not None:
            self.reset(vec)
        if allow is not None:
            self.set_filter(_allow_words(self.num_rows, allow))
        if groups is not None:
            self.set_groups(groups)

    def run_filtered(self, vec=None, allow=None):
        """One filtered query with host arrays: reset(vec) if given, set_filter(allow) if given (a bool array of length rows, or
        row_mask() words), then the query restricted to the installed mask. Returns (values, indices) like read_result."""
        self._install(vec, allow)
        self.enqueue_filtered(0, 1, 0)
        self.synchronize()
        return self.read_result()

    def set_groups(self, groups, n_groups=None):
        """Installs the group labels of grouped queries: groups[r] < n_groups for every local row r (n_groups None: the largest
        label + 1); None removes them. A label >= n_groups raises TkspmvError(ERR_INVALID) and installs nothing."""
        if groups is None:
            _lib.check(_lib.lib().tkspmv_set_groups(self._h, None, 0))
            self._n_groups = 0
            return
        g = np.asarray(groups)
        if g.shape != (self.num_rows,):
            raise ValueError(f"groups has shape {g.shape}, expected ({self.num_rows},)")
        if g.size and (g.min() < 0 or g.max() > 0xFFFFFFFF):
            raise ValueError("group labels must be uint32 values")
        g = np.ascontiguousarray(g, dtype=np.uint32)
        if n_groups is None:
            n_groups = int(g.max()) + 1 if g.size else 1
        _lib.check(_lib.lib().tkspmv_set_groups(self._h, u32p(g), int(n_groups)))
        self._n_groups = int(n_groups)  # (run_facets sizes its arrays by it)

    def enqueue_grouped(self, dev_xs, count, dev_mask=0, mask_stride=0, dev_idx=0, dev_val=0, dev_grp=0, dev_n=0, stream=0):
        """Grouped top-k of `count` queries (dev_xs + i*cols; dev_xs = 0 with count = 1: the vector installed by reset()): the k best
        groups of set_groups(), each by its best row. dev_mask: allow-mask(s) as in enqueue_filtered, 0 = unfiltered. dev_idx /
        dev_val / dev_grp: [count][k] device buffers, all three or none (engine buffers, last query wins); dev_n: [count] real
        entries per list (optional). Pads are (0, 0.0) with group id 0xFFFFFFFF. No host sync; one grouped call in flight at a time."""
        _lib.check(_lib.lib().tkspmv_enqueue_grouped(self._h, ptr(dev_xs), int(count), ptr(dev_mask), int(mask_stride), ptr(dev_idx), ptr(dev_val),
                                                     ptr(dev_grp), ptr(dev_n), ptr(stream)))

    def run_grouped(self, vec=None, allow=None, groups=None):
        """One grouped query with host arrays: reset(vec) if given, set_filter(allow) if given (a bool array of length rows, or
        row_mask() words; the query is then restricted to it), set_groups(groups) if given. Returns (values, indices, groups) of
        the groups that exist for the query, at most k, ordered like read_result."""
        self._install(vec, allow, groups)
        return self._run_grouped(allow is not None)

    def _run_grouped(self, use_filter, boosted=False):
        idx = np.zeros(self.k, dtype=np.uint32)
        val = np.zeros(self.k, dtype=np.float32)
        grp = np.zeros(self.k, dtype=np.uint32)
        n = C.c_int32(0)
        run = _lib.lib().tkspmv_run_boosted_grouped if boosted else _lib.lib().tkspmv_run_grouped
        _lib.check(run(self._h, int(use_filter), u32p(idx), f32p(val), u32p(grp), C.byref(n)))
        return val[:n.value], idx[:n.value], grp[:n.value]

    def enqueue_after(self, dev_xs, count, dev_cursors=0, dev_mask=0, mask_stride=0, dev_idx=0, dev_val=0, dev_n=0, dev_total=0, dev_next=0,
                      stream=0):
        """Search-after paging of `count` queries (dev_xs + i*cols; dev_xs = 0 with count = 1: the vector installed by reset()): the
        first k eligible rows that rank strictly behind dev_cursors[i] (_lib.Cursor records in device memory, read in stream
        order; 0 = from the top for every query). dev_mask: allow-mask(s) as in enqueue_filtered, 0 = unfiltered. dev_idx / dev_val:
        [count][k] device buffers, both or none (engine buffers, last query wins); dev_n / dev_total: [count] real entries per
        page and eligible rows behind the cursor, the page included (optional); dev_next: [count] cursors of the following pages
        (optional; may be dev_cursors itself: the same call again then walks on). Pads are (0, 0.0). No host sync; one such call
        in flight at a time; the first call allocates about 12 bytes per row."""
        _lib.check(_lib.lib().tkspmv_enqueue_after(self._h, ptr(dev_xs), int(count), ptr(dev_cursors), ptr(dev_mask), int(mask_stride), ptr(dev_idx),
                                                   ptr(dev_val), ptr(dev_n), ptr(dev_total), ptr(dev_next), ptr(stream)))

    def run_after(self, cursor=None, vec=None, allow=None):
        """One page with host arrays: reset(vec) if given, set_filter(allow) if given (a bool array of length rows, or row_mask()
        words; the query is then restricted to it), then the k eligible rows behind `cursor` -- None (from the top) or
        (row, score_bits, state), as the call before returned it. Returns (idx, val, n, total, next): idx / val of k entries, the
        first n real, the rest pads; total = the eligible rows behind the cursor, this page included; next = the cursor of the
        following page, state CURSOR_END when this page was the last."""
        self._install(vec, allow)
        return self._run_after(cursor, allow is not None)

    def _run_after(self, cursor, use_filter, boosted=False):
        cur = None
        if cursor is not None:
            row, bits, state = (int(v) for v in cursor)
            cur = C.byref(_lib.Cursor(row, bits, state, 0))
        idx = np.zeros(self.k, dtype=np.uint32)
        val = np.zeros(self.k, dtype=np.float32)
        n, total, nxt = C.c_int32(0), C.c_uint32(0), _lib.Cursor()
        run = _lib.lib().tkspmv_run_boosted if boosted else _lib.lib().tkspmv_run_after
        _lib.check(run(self._h, cur, int(use_filter), u32p(idx), f32p(val), C.byref(n), C.byref(total), C.byref(nxt)))
        return idx, val, int(n.value), int(total.value), (int(nxt.row), int(nxt.score_bits), int(nxt.state))

    def pages(self, vec=None, allow=None):
        """Generator over the complete ranking of the eligible rows, page by page (reset(vec) / set_filter(allow) first, as in
        run_after): yields (values, indices) of each page's real entries, ordered like read_result, until the cursor says END --
        no empty trailing page, and no page at all when no row is eligible. The query vector and the mask must stay installed
        while the generator is in use."""
        yield from self._pages(self.run_after(None, vec, allow), allow is not None, False)

    def _pages(self, page, use_filter, boosted):
        """The walk behind pages() and boosted_pages(): from the first page (run_after's tuple) on until the cursor says END."""
        idx, val, n, _, cursor = page
        while n:
            yield val[:n], idx[:n]
            if cursor[2] == _lib.CURSOR_END:
                return
            idx, val, n, _, cursor = self._run_after(cursor, use_filter, boosted)

    def set_boost(self, weight=None, bias=None):
        """Installs the boost of boosted queries: float32 weight[r] and bias[r] for every local row r, either may be None (no
        multiply / no add); both None removes it. The boosted score of a row is weight[r] * score + bias[r], two separately
        rounded float32 operations (host.boost_scores restates it). An entry that is not finite raises TkspmvError(ERR_INVALID) and
        installs nothing."""
        arrays = []
        for name, a in (("weight", weight), ("bias", bias)):
            if a is not None:
                if np.shape(a) != (self.num_rows,):
                    raise ValueError(f"{name} has shape {np.shape(a)}, expected ({self.num_rows},)")
                a = np.ascontiguousarray(a, dtype=np.float32)
            arrays.append(a)
        _lib.check(_lib.lib().tkspmv_set_boost(self._h, *(f32p(a) for a in arrays)))

    def set_cosine(self):
        """Installs the cosine weights 1 / ||row r||_2 (row_stats(ROW_INV_L2)) as the boost and removes any installed bias: the state
        of set_boost(weight=w), with w computed on the device from the matrix the engine holds -- no COO needed, so engines made by
        from_packed have it too. With a query of norm 1, run_boosted() then returns cosines. The sums of squares are float32 in the
        engine's own order (host.cosine_weights sums in float64: the weights can differ in the last bits)."""
        _lib.check(_lib.lib().tkspmv_set_boost_cosine(self._h))

    def enqueue_boosted(self, dev_xs, count, dev_weight=0, dev_bias=0, boost_stride=0, dev_cursors=0, dev_mask=0, mask_stride=0, dev_idx=0,
                        dev_val=0, dev_n=0, dev_total=0, dev_next=0, stream=0):
        """enqueue_after over boosted scores: query i reads float32 dev_weight + i*boost_stride and dev_bias + i*boost_stride
        (device arrays of rows floats by local row; the stride in floats, 0 = one pair for every query; either may be 0: no
        multiply / no add; both 0: the boost installed by set_boost). Every other argument and the outputs are enqueue_after's,
        read on the boosted score: the cursors' score_bits are boosted scores, and min_score applies to them. No host sync; one
        enqueue_after or enqueue_boosted call in flight at a time (they share their scratch)."""
        _lib.check(_lib.lib().tkspmv_enqueue_boosted(self._h, ptr(dev_xs), int(count), ptr(dev_weight), ptr(dev_bias), int(boost_stride),
                                                     ptr(dev_cursors), ptr(dev_mask), int(mask_stride), ptr(dev_idx), ptr(dev_val), ptr(dev_n),
                                                     ptr(dev_total), ptr(dev_next), ptr(stream)))

    def run_boosted(self, cursor=None, vec=None, allow=None, weight=None, bias=None):
        """run_after over boosted scores: reset(vec) / set_filter(allow) if given, set_boost(weight, bias) if either is given
        (else the boost installed before), then the k eligible rows behind `cursor` in the order of the boosted scores. Returns
        run_after's tuple (idx, val, n, total, next); val holds boosted scores."""
        self._install(vec, allow)
        if weight is not None or bias is not None:
            self.set_boost(weight, bias)
        return self._run_after(cursor, allow is not None, True)

    def boosted_pages(self, vec=None, allow=None, weight=None, bias=None):
        """pages() over boosted scores (arguments as in run_boosted): yields (values, indices) of each page's real entries until the
        cursor says END. The query vector, the mask and the boost must stay installed while the generator is in use."""
        yield from self._pages(self.run_boosted(None, vec, allow, weight, bias), allow is not None, True)

    def enqueue_range(self, dev_xs, count, dev_thresholds, dev_counts, dev_idx=0, dev_val=0, capacity=0, dev_mask=0, mask_stride=0, stream=0):
        """Range queries: for query i (dev_xs + i*cols; dev_xs = 0 with count = 1: the vector installed by reset()) every row that
        has entries, is allowed by dev_mask + i*mask_stride words (0: unfiltered) and scores >= dev_thresholds[i]. dev_counts[i]
        receives the number of matches; dev_idx / dev_val + i*capacity the first min(count, capacity) of them, in no particular
        order (capacity = 0 with no outputs: count only). No host sync, no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_range(self._h, ptr(dev_xs), int(count), ptr(dev_thresholds), ptr(dev_mask), int(mask_stride),
                                                   ptr(dev_idx), ptr(dev_val), int(capacity), ptr(dev_counts), ptr(stream)))

    def _run_range(self, threshold, use_filter, capacity, boosted=False):
        idx = np.zeros(max(capacity, 1), dtype=np.uint32)
        val = np.zeros(max(capacity, 1), dtype=np.float32)
        count = C.c_uint64(0)
        run = _lib.lib().tkspmv_run_boosted_range if boosted else _lib.lib().tkspmv_run_range
        _lib.check(run(self._h, float(threshold), int(use_filter), u32p(idx) if capacity else None, f32p(val) if capacity else None, int(capacity),
                       C.byref(count)))
        n = min(int(count.value), capacity)
        return val[:n], idx[:n], int(count.value)

    def run_range(self, threshold, vec=None, allow=None, capacity=None):
        """One range query with host arrays: reset(vec) if given, set_filter(allow) if given (a bool array of length rows, or
        row_mask() words; the query is then restricted to it), then every row scoring >= threshold. Returns (values, indices)
        sorted like read_result. capacity=None: the count is asked for first, then exactly that many (the set is deterministic);
        else at most `capacity` matches are returned and last_range_count holds the true number."""
        self._install(vec, allow)
        use_filter = allow is not None
        if capacity is None:
            _, _, capacity = self._run_range(threshold, use_filter, 0)
        val, idx, self.last_range_count = self._run_range(threshold, use_filter, int(capacity))
        return val, idx

    def _install_boost(self, vec, allow, groups, weight, bias):
        """The prologue of the boosted host-array forms: _install, then set_boost(weight, bias) if either is given (else the boost
        installed before stays)."""
        self._install(vec, allow, groups)
        if weight is not None or bias is not None:
            self.set_boost(weight, bias)

    def enqueue_boosted_range(self, dev_xs, count, dev_thresholds, dev_counts, dev_weight=0, dev_bias=0, boost_stride=0, dev_idx=0, dev_val=0,
                              capacity=0, dev_mask=0, mask_stride=0, stream=0):
        """enqueue_range over boosted scores: query i reads dev_weight / dev_bias + i*boost_stride as in enqueue_boosted (either may
        be 0; both 0: the boost installed by set_boost), and a row matches when its boosted score s' is above -inf and >=
        dev_thresholds[i] (min_score plays no part). dev_counts[i] receives the number of matches; dev_idx / dev_val + i*capacity
        the first min(count, capacity) of them as (row id, s'), in no particular order. Per query the scores kernel and one pass
        over its scores. No host sync; one enqueue_after / enqueue_boosted / enqueue_boosted_range / enqueue_boosted_facets call in
        flight at a time (they share their scratch)."""
        _lib.check(_lib.lib().tkspmv_enqueue_boosted_range(self._h, ptr(dev_xs), int(count), ptr(dev_weight), ptr(dev_bias), int(boost_stride),
                                                           ptr(dev_thresholds), ptr(dev_mask), int(mask_stride), ptr(dev_idx), ptr(dev_val),
                                                           int(capacity), ptr(dev_counts), ptr(stream)))

    def run_boosted_range(self, threshold, vec=None, allow=None, weight=None, bias=None, capacity=None):
        """run_range over boosted scores: reset(vec) / set_filter(allow) if given, set_boost(weight, bias) if either is given (else
        the boost installed before, e.g. by set_cosine()), then every row whose boosted score is >= threshold. Returns (values,
        indices) sorted like read_result; values are boosted scores. capacity as in run_range (last_range_count holds the true
        number). host.boosted_matches restates the contract."""
        self._install_boost(vec, allow, None, weight, bias)
        use_filter = allow is not None
        if capacity is None:
            _, _, capacity = self._run_range(threshold, use_filter, 0, True)
        val, idx, self.last_range_count = self._run_range(threshold, use_filter, int(capacity), True)
        return val, idx

    def enqueue_match(self, dev_clauses, dev_preds, count, dev_out, out_stride=0, dev_counts=0, clause_stride=0, dev_mask=0, mask_stride=0, stream=0):
        """Term predicates: for query i the allow-mask of the rows whose own columns satisfy dev_preds[i] (_lib.Match records in device
        memory) under the clause table dev_clauses + i*clause_stride words (uint32[cols] as bool_query() builds it; 0: one table for
        every query), restricted to dev_mask + i*mask_stride words (0: unfiltered). dev_out + i*out_stride receives the mask's
        ceil(rows/32) words (out_stride = 0 with count = 1), valid wherever a mask is accepted; dev_counts[i] (optional) the number of
        matching rows. No host sync, no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_match(self._h, ptr(dev_clauses), int(clause_stride), ptr(dev_preds), int(count), ptr(dev_mask),
                                                   int(mask_stride), ptr(dev_out), int(out_stride), ptr(dev_counts), ptr(stream)))

    def match(self, clauses, pred, allow=None, install=False):
        """One term predicate with host arrays: clauses (uint32[cols]) and pred (must, must_not, should, min_should) as bool_query()
        returns them; set_filter(allow) first if given (a bool array of length rows, or row_mask() words; the result is then
        restricted to it). Returns (mask_words, count): the allow-mask of the matching rows, as row_mask() would pack it, and their
        number. install=True: the result becomes the engine's installed filter (set_filter's), without leaving the device."""
        t = np.ascontiguousarray(clauses, dtype=np.uint32)
        if t.shape != (self.num_cols,):
            raise ValueError(f"clause table has shape {t.shape}, expected ({self.num_cols},)")
        self._install(allow=allow)
        rec = _lib.Match(*(int(v) & 0xFFFFFFFF for v in pred))
        words = np.zeros(max(1, (self.num_rows + 31) // 32), dtype=np.uint32)
        count = C.c_uint64(0)
        _lib.check(_lib.lib().tkspmv_run_match(self._h, u32p(t), C.byref(rec), int(allow is not None), int(bool(install)), u32p(words),
                                               C.byref(count)))
        return words, int(count.value)

    def enqueue_facets(self, dev_xs, count, dev_thresholds, dev_counts, n_bins=0, dev_labels=0, dev_best=0, dev_totals=0, dev_mask=0, mask_stride=0,
                       stream=0):
        """Facet counts: for query i (dev_xs, dev_thresholds, dev_mask / mask_stride as in enqueue_range) the matches per label.
        dev_labels: [rows] uint32 labels of the local rows with n_bins bins (a label >= n_bins: no bin); 0 with n_bins = 0: the
        labels of set_groups(). dev_counts[i*n_bins + b] receives the matches with label b; dev_best (optional, _lib.FacetBest
        records) each bin's match that comes first in the result order, (0, 0) for an empty bin; dev_totals[i] (optional) all
        matches. No host sync, no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_facets(self._h, ptr(dev_xs), int(count), ptr(dev_thresholds), ptr(dev_mask), int(mask_stride),
                                                    ptr(dev_labels), int(n_bins), ptr(dev_counts), ptr(dev_best), ptr(dev_totals), ptr(stream)))

    def run_facets(self, threshold, vec=None, allow=None, groups=None):
        """One facet query with host arrays: reset(vec) if given, set_filter(allow) if given (a bool array of length rows, or
        row_mask() words; the query is then restricted to it), set_groups(groups) if given, then the rows scoring >= threshold
        counted per installed label. Returns (counts, best_idx, best_val, total): per group its matches and the row id and score
        of its best match ((0, 0.0) for a group without one), and the number of all matches."""
        self._install(vec, allow, groups)
        return self._run_facets(threshold, allow is not None)

    def _run_facets(self, threshold, use_filter, boosted=False):
        n = max(1, self._n_groups)  # (none installed: the library says so and writes nothing)
        counts = np.zeros(n, dtype=np.uint32)
        records = (_lib.FacetBest * n)()
        total = C.c_uint64(0)
        run = _lib.lib().tkspmv_run_boosted_facets if boosted else _lib.lib().tkspmv_run_facets
        _lib.check(run(self._h, float(threshold), int(use_filter), u32p(counts), records, C.byref(total)))
        best = np.frombuffer(records, dtype=np.uint32).reshape(n, 2)
        n = self._n_groups
        return counts[:n], best[:n, 0].copy(), best[:n, 1].copy().view(np.float32), int(total.value)

    def enqueue_boosted_facets(self, dev_xs, count, dev_thresholds, dev_counts, dev_weight=0, dev_bias=0, boost_stride=0, n_bins=0, dev_labels=0,
                               dev_best=0, dev_totals=0, dev_mask=0, mask_stride=0, stream=0):
        """enqueue_facets over boosted scores: the match rule of enqueue_boosted_range, the outputs of enqueue_facets (dev_best
        holds boosted scores). The expectation is host.facet_counts(sb, ok, ...) with sb = host.boost_scores(y, w, b) and ok =
        present & allow & (sb > -inf). No host sync; shares the scratch of enqueue_boosted_range."""
        _lib.check(_lib.lib().tkspmv_enqueue_boosted_facets(self._h, ptr(dev_xs), int(count), ptr(dev_weight), ptr(dev_bias), int(boost_stride),
                                                            ptr(dev_thresholds), ptr(dev_mask), int(mask_stride), ptr(dev_labels), int(n_bins),
                                                            ptr(dev_counts), ptr(dev_best), ptr(dev_totals), ptr(stream)))

    def run_boosted_facets(self, threshold, vec=None, allow=None, groups=None, weight=None, bias=None):
        """run_facets over boosted scores: the prologue of run_facets, set_boost(weight, bias) if either is given (else the boost
        installed before), then the rows whose boosted score is >= threshold counted per installed label. Returns run_facets'
        tuple; best_val holds boosted scores. The expectation is host.facet_counts(sb, ok, ...) with sb = host.boost_scores(y, w,
        b) and ok = present & allow & (sb > -inf)."""
        self._install_boost(vec, allow, groups, weight, bias)
        return self._run_facets(threshold, allow is not None, True)

    def enqueue_boosted_grouped(self, dev_xs, count, dev_weight=0, dev_bias=0, boost_stride=0, dev_mask=0, mask_stride=0, dev_idx=0, dev_val=0,
                                dev_grp=0, dev_n=0, stream=0):
        """enqueue_grouped over boosted scores (dev_weight / dev_bias / boost_stride as in enqueue_boosted): eligibility (min_score),
        each group's representative, the order and the returned values all go by the boosted score. The expectation is
        host.collapse_topk(sb, ok, ...) with sb = host.boost_scores(y, w, b) and ok = present & allow & (sb > -inf). No host sync;
        one enqueue_grouped or enqueue_boosted_grouped call in flight at a time."""
        _lib.check(_lib.lib().tkspmv_enqueue_boosted_grouped(self._h, ptr(dev_xs), int(count), ptr(dev_weight), ptr(dev_bias), int(boost_stride),
                                                             ptr(dev_mask), int(mask_stride), ptr(dev_idx), ptr(dev_val), ptr(dev_grp), ptr(dev_n),
                                                             ptr(stream)))

    def run_boosted_grouped(self, vec=None, allow=None, groups=None, weight=None, bias=None):
        """run_grouped over boosted scores: the prologue of run_grouped, set_boost(weight, bias) if either is given (else the boost
        installed before). Returns (values, indices, groups) like run_grouped; values are boosted scores. The expectation is
        host.collapse_topk(sb, ok, ...) with sb = host.boost_scores(y, w, b) and ok = present & allow & (sb > -inf)."""
        self._install_boost(vec, allow, groups, weight, bias)
        return self._run_grouped(allow is not None, True)

    def enqueue_row_vectors(self, dev_rows, count, dev_xs, dev_len=0, stream=0):
        """Stored rows as dense query vectors: dev_rows[i] (uint32, a GLOBAL row id as queries return them) is expanded into
        dev_xs + i*cols (float32: zeros, and the row's values at their columns; a repeated column holds the fp32 sum of its entries
        in order). dev_len[i] (optional) receives the row's number of entries, 0xFFFFFFFF for an id outside the engine's rows (a
        zero vector). The output feeds enqueue_batch / enqueue_filtered / enqueue_range / enqueue_multi unchanged. No host sync, no
        engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_row_vectors(self._h, ptr(dev_rows), int(count), ptr(dev_xs), ptr(dev_len), ptr(stream)))

    def row_vectors(self, rows):
        """enqueue_row_vectors with host arrays: (xs[n, cols] float32, lengths[n] uint32) of the given global row ids. Waits."""
        ids = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        xs = np.empty((ids.size, self.num_cols), dtype=np.float32)
        ln = np.empty(ids.size, dtype=np.uint32)
        if ids.size:
            _lib.check(_lib.lib().tkspmv_row_vectors(self._h, u32p(ids), int(ids.size), f32p(xs), u32p(ln)))
        return xs, ln

    def similar(self, rows, exclude_self=False):
        """More-like-this: for every given global row id the engine's top-k with that row as the query, (values[n, k], indices[n, k]),
        each list ordered like read_result. exclude_self: the row itself leaves its list (the rest moves up, the last slot becomes
        the pad (0, 0.0)); to get k others create the engine with k + 1. Waits."""
        ids = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        idx = np.zeros((ids.size, self.k), dtype=np.uint32)
        val = np.zeros((ids.size, self.k), dtype=np.float32)
        if ids.size:
            _lib.check(_lib.lib().tkspmv_run_similar(self._h, u32p(ids), int(ids.size), int(bool(exclude_self)), u32p(idx), f32p(val)))
        return val, idx

    def enqueue_score_rows(self, dev_xs, count, dev_rows, n_rows, dev_scores, rows_stride=0, stream=0):
        """Scores of given rows: dev_scores[q*n_rows + i] (float32) = what row dev_rows[q*rows_stride + i] (uint32, a GLOBAL row id as
        queries return them; rows_stride = 0: one list for every query) scores for query q (dev_xs + q*cols; dev_xs = 0 with
        count = 1: the vector installed by reset()), bit for bit the value every other path reports. Computed from the rows' own
        packets: the matrix is not streamed. A row without entries scores +0.0, an id outside the engine's rows -inf. No host sync,
        no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_score_rows(self._h, ptr(dev_xs), int(count), ptr(dev_rows), int(n_rows), int(rows_stride),
                                                        ptr(dev_scores), ptr(stream)))

    def score_rows(self, rows, vecs=None):
        """enqueue_score_rows with host arrays: float32[count, n_rows] scores of the given global row ids. rows: 1-D (one list for
        every query) or [count, n_rows] (a list per query); vecs: [count, cols] (or one vector of cols), None: the vector installed
        by reset(). Waits."""
        ids = np.ascontiguousarray(rows, dtype=np.uint32)
        if ids.ndim not in (1, 2):
            raise ValueError("rows must be a 1-D list or a [count, n_rows] array")
        xs = None
        if vecs is not None:
            xs = np.ascontiguousarray(vecs, dtype=np.float32)
            xs = xs.reshape(1, -1) if xs.ndim == 1 else xs
            if xs.ndim != 2 or xs.shape[1] != self.num_cols:
                raise ValueError(f"query vectors must be [count, {self.num_cols}]")
        count = 1 if xs is None else int(xs.shape[0])
        if ids.ndim == 2 and ids.shape[0] != count:
            raise ValueError(f"rows has {ids.shape[0]} lists for {count} queries")
        n_rows = int(ids.shape[-1])
        out = np.empty((count, n_rows), dtype=np.float32)
        if count and n_rows:
            _lib.check(_lib.lib().tkspmv_score_rows(self._h, f32p(xs), count, u32p(ids), n_rows, n_rows if ids.ndim == 2 else 0, f32p(out)))
        return out

    def enqueue_row_stats(self, kind, dev_out, stream=0):
        """Row statistics: dev_out[r] (float32, rows of them, by LOCAL row) = one statistic of row r, kind = _lib.ROW_NNZ (stored
        entries), ROW_L1 (sum of |v|), ROW_L2SQ (sum of v*v) or ROW_INV_L2 (the cosine weight 1/sqrt(L2SQ); 0.0 where that sum is 0,
        inf or NaN). The sums are float32 in the order every streaming path sums a row's score in; a row without entries gives
        +0.0. One pass over the matrix. No host sync, no engine state touched. ROW_INV_L2 or ROW_NNZ in a device array of the
        caller's is what per-query or combined weights for enqueue_boosted(dev_weight=...) are made from."""
        _lib.check(_lib.lib().tkspmv_enqueue_row_stats(self._h, int(kind), ptr(dev_out), ptr(stream)))

    def row_stats(self, kind):
        """enqueue_row_stats with a host array: float32[rows] of the given kind. Waits."""
        out = np.empty(max(self.num_rows, 1), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_row_stats(self._h, int(kind), f32p(out)))
        return out[:self.num_rows]

    def enqueue_assign(self, dev_xs, count, dev_labels, dev_best=0, stream=0):
        """Assignment: for every LOCAL row r the best-scoring of the `count` vectors at dev_xs (float32, cols each, back to back):
        dev_labels[r] (uint32) = its index, ties to the smallest, and dev_best[r] (float32, optional) = that score, bit for bit the
        value every other path reports for the row and the vector. A row without entries gets label 0 and +0.0. One pass over the
        matrix per 16384 / column tier vectors (16 at up to 1024 columns, 4 up to 4096, 1 beyond); dev_best = 0 only with at most
        that many vectors. No host sync, no engine state touched. The labels are what set_groups, enqueue_facets(dev_labels=...)
        and the masks of enqueue_col_stats are made from."""
        _lib.check(_lib.lib().tkspmv_enqueue_assign(self._h, ptr(dev_xs), int(count), ptr(dev_labels), ptr(dev_best), ptr(stream)))

    def assign(self, vecs, install=False):
        """enqueue_assign with host arrays: (labels uint32[rows], best float32[rows]) for vecs[count, cols] (or one vector of cols).
        Waits. install: the labels become the engine's group labels, set_groups(labels, n_groups=count) -- run_grouped then returns
        each cluster once, run_facets counts per cluster."""
        xs = _vectors(vecs, self.num_cols)
        labels = np.empty(max(self.num_rows, 1), dtype=np.uint32)
        best = np.empty(max(self.num_rows, 1), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_assign(self._h, f32p(xs), int(xs.shape[0]), u32p(labels), f32p(best)))
        labels, best = labels[:self.num_rows], best[:self.num_rows]
        if install:
            self.set_groups(labels, n_groups=int(xs.shape[0]))
        return labels, best

    def enqueue_label_sums(self, dev_labels, n_bins, exp, dev_sums, mode=_lib.SUMS_RAW, dev_out=0, flags=0, stream=0):
        """Label sums: dev_sums[b][c] (int64, [n_bins][cols]) = the sum of quantise(v, exp) over the stored entries (r, c, v) of the
        LOCAL rows with dev_labels[r] == b (uint32 labels; one >= n_bins has no bin; dev_labels = 0 with n_bins = 0: the labels
        set_groups installed). Integers added with integer atomics: exact with respect to host.quantise and bit-identical whatever
        the geometry or sharding, so the sums of shards taken with one common exp simply add up. mode _lib.SUMS_FLOAT / SUMS_UNIT
        adds the closing launch into dev_out (float32 [n_bins][cols]): the sums as floats, or scaled to unit length -- a bin without
        a norm is then NOT written, so dev_out holding the previous centroids keeps them: enqueue_assign followed by
        enqueue_label_sums(SUMS_UNIT, dev_out = the vectors of the next assign) is one k-means iteration in stream order. flags:
        _lib.SUMS_ACCUMULATE adds to what dev_sums holds; SUMS_SINK_LDS / SUMS_SINK_DIRECT force one of the kernel's sinks. No host
        sync, no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_label_sums(self._h, ptr(dev_labels), int(n_bins), int(exp), int(flags), ptr(dev_sums), int(mode), ptr(dev_out),
                                                        ptr(stream)))

    def enqueue_sums_close(self, dev_sums, n_bins, exp, mode, dev_out, stream=0):
        """The closing launch of enqueue_label_sums alone (mode SUMS_FLOAT or SUMS_UNIT) over int64 sums the caller holds, e.g. the
        integer sum of the shards' sums. No host sync."""
        _lib.check(_lib.lib().tkspmv_enqueue_sums_close(self._h, ptr(dev_sums), int(n_bins), int(exp), int(mode), ptr(dev_out), ptr(stream)))

    def sums_exponent(self):
        """The default exponent of label sums: no sum can reach 2^63 with it, and the largest values are summed exactly (from three
        col_stats passes; waits). Shards whose sums are merged must share one exponent: the maximum of theirs."""
        e = C.c_int32()
        _lib.check(_lib.lib().tkspmv_sums_exponent(self._h, C.byref(e)))
        return int(e.value)

    def label_sums(self, labels=None, n_bins=None, mode=_lib.SUMS_RAW, exp=None, out=None):
        """enqueue_label_sums with host arrays: (sums int64[n_bins, cols], floats float32[n_bins, cols] or None with SUMS_RAW).
        labels = None: the labels and bin count set_groups (or assign(install=True)) installed; exp = None: sums_exponent(). out:
        with SUMS_UNIT the rows that bins without a norm keep (zeros without it). Waits."""
        if labels is None:
            lab, n_bins = None, int(getattr(self, "_n_groups", 0) if n_bins is None else n_bins)
        else:
            lab = np.ascontiguousarray(labels, dtype=np.uint32).ravel()
            if lab.shape != (self.num_rows,):
                raise ValueError(f"labels must have shape ({self.num_rows},)")
            n_bins = int(lab.max()) + 1 if n_bins is None and lab.size else int(n_bins or 1)
            lab = lab if lab.size else np.zeros(1, dtype=np.uint32)
        exp = self.sums_exponent() if exp is None else int(exp)
        cols = self.num_cols
        sums = np.zeros((max(n_bins, 1), max(cols, 1)), dtype=np.int64)
        res = None
        if int(mode) != _lib.SUMS_RAW:
            res = np.zeros((n_bins, cols), dtype=np.float32) if out is None else np.array(out, dtype=np.float32).reshape(n_bins, cols)
        _lib.check(_lib.lib().tkspmv_label_sums(self._h, u32p(lab), 0 if lab is None else n_bins, exp, int(mode), _lib.i64p(sums), f32p(res)))
        return sums.reshape(-1)[:n_bins * cols].reshape(n_bins, cols), res

    def kmeans(self, cent, iters):
        """Spherical k-means on the device: `iters` times enqueue_assign against the centroids, then enqueue_label_sums(SUMS_UNIT)
        into the centroid buffer itself -- a cluster that ends empty keeps its vector --, then one final assignment; the centroids
        never visit the host in between. cent: float32[count, cols] start vectors. Returns (cent float32[count, cols], labels
        uint32[rows], best float32[rows]): the final centroids and every row's assignment to them. Waits."""
        import torch
        xs = _vectors(cent, self.num_cols, what="centroids")
        count, exp = int(xs.shape[0]), self.sums_exponent()
        dev = torch.device("cuda", int(self.info()["device"]))
        d_xs = torch.from_numpy(xs).to(dev)
        d_lab = torch.zeros(max(self.num_rows, 1), dtype=torch.int32, device=dev)
        d_best = torch.zeros(max(self.num_rows, 1), dtype=torch.float32, device=dev)
        d_sums = torch.zeros(count * max(self.num_cols, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        for it in range(int(iters) + 1):
            self.enqueue_assign(d_xs.data_ptr(), count, d_lab.data_ptr(), d_best.data_ptr())
            if it < int(iters):
                self.enqueue_label_sums(d_lab.data_ptr(), count, exp, d_sums.data_ptr(), _lib.SUMS_UNIT, d_xs.data_ptr())
        self.synchronize()
        return d_xs.cpu().numpy(), d_lab.cpu().numpy().view(np.uint32)[:self.num_rows], d_best.cpu().numpy()[:self.num_rows]

    def enqueue_nearest(self, dev_xs, count, n, dev_labels, dev_scores, dev_mask=0, stream=0):
        """Nearest-n assignment: for every LOCAL row r its n best-scoring of the `count` vectors at dev_xs (float32, cols each, back to
        back), in order -- score descending, ties to the smaller index --: dev_labels[r, j] (uint32) and dev_scores[r, j] (float32),
        rows x n each, row-major, the scores bit for bit what every other path reports. 1 <= n <= _lib.NEAREST_MAX_N. Entries beyond
        count are (_lib.NEAREST_NONE, -inf). dev_mask (row_mask() words on the device, 0: every row) restricts the rows: a row outside
        it is (NEAREST_NONE, -inf) throughout, so its label falls into no bin of enqueue_label_sums or enqueue_facets. A row without
        entries gets labels 0, 1, .. with +0.0. n = 1 without a mask is enqueue_assign. One pass over the matrix per 16384 / column
        tier vectors. No host sync, no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_nearest(self._h, ptr(dev_xs), int(count), int(n), ptr(dev_mask), ptr(dev_labels), ptr(dev_scores), ptr(stream)))

    def nearest(self, vecs, n, mask=None):
        """enqueue_nearest with host arrays: (labels uint32[rows, n], scores float32[rows, n]) for vecs[count, cols] (or one vector of
        cols). mask None: every row; True: the rows of the mask set_filter() installed; a bool array of length rows or row_mask()
        words: installed with set_filter() first, as run_filtered does. host.margin(scores) is each row's s1 - s2. Waits."""
        xs, n = _vectors(vecs, self.num_cols), int(n)
        if mask is not None and mask is not True:
            self._install(allow=mask)
        labels = np.empty((max(self.num_rows, 1), max(n, 1)), dtype=np.uint32)
        scores = np.empty((max(self.num_rows, 1), max(n, 1)), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_nearest(self._h, f32p(xs), int(xs.shape[0]), n, int(mask is not None), u32p(labels), f32p(scores)))
        return labels[:self.num_rows], scores[:self.num_rows]

    def enqueue_col_stats(self, kind, out, masks=None, mask_stride=0, out_stride=0, stream=None, count=1):
        """Column statistics: one 4-byte word per column and set of rows into device memory at `out` -- kind = _lib.COL_NNZ (uint32:
        the stored entries of the column; explicit zeros and a column repeated within a row count), COL_MAX / COL_MIN (float32: the
        largest / smallest stored value, -inf / +inf for a column without an entry). masks = None: one set, all rows. Else `count`
        sets, set i the rows of the allow-mask at masks + i*mask_stride words (row_mask() words by LOCAL row; stride 0: the same mask),
        written at out + i*out_stride words (>= cols when count > 1). Exact and bit-reproducible; one pass over the matrix per set.
        No host sync, no engine state touched."""
        _lib.check(_lib.lib().tkspmv_enqueue_col_stats(self._h, int(kind), int(count), ptr(masks), int(mask_stride), ptr(out), int(out_stride),
                                                       ptr(stream)))

    def col_stats(self, kind, use_filter=False):
        """enqueue_col_stats with a host array: uint32[cols] (COL_NNZ) or float32[cols] (COL_MAX, COL_MIN) over all rows, or with
        use_filter among the rows of the mask set_filter() installed. Waits."""
        out = np.empty(max(self.num_cols, 1), dtype=np.uint32)
        _lib.check(_lib.lib().tkspmv_col_stats(self._h, int(kind), int(bool(use_filter)), ptr(out.ctypes.data)))
        out = out[:self.num_cols]
        return out if int(kind) == _lib.COL_NNZ else out.view(np.float32)

    def rerank(self, rows, vec=None, k=None):
        """The given global row ids re-scored for one query (vec; None: the vector installed by reset()) and ordered like
        read_result -- score descending, then row descending: (values, indices). Ids outside the engine's rows are dropped; at most
        k are returned if k is given. The scores come from score_rows, the sorting runs on the host."""
        ids = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        ids = ids[(ids.astype(np.int64) >= self.first_row) & (ids.astype(np.int64) < self.first_row + self.num_rows)]
        val = self.score_rows(ids, vec)[0] if ids.size else np.empty(0, dtype=np.float32)
        order = np.lexsort((-ids.astype(np.int64), -val.astype(np.float64)))
        if k is not None:
            order = order[:int(k)]
        return val[order], ids[order]

    def enqueue_multi(self, dev_xs, count, dev_idx=0, dev_val=0, stream=0):
        """enqueue_batch with several queries per pass over the matrix (info()["multi_q"] of them share every chunk that
        is loaded; engine created with multi_q > 0). Same arguments; dev_xs = 0 with count = 1: the vector installed by
        reset(). No host sync."""
        _lib.check(_lib.lib().tkspmv_enqueue_multi(self._h, ptr(dev_xs), int(count), ptr(dev_idx), ptr(dev_val), ptr(stream)))

    def time_multi(self, dev_xs, n_x, iters):
        """ns per query of `iters` queries through the multi-query path (one hipEvent pair around the sequence)."""
        ns = C.c_double()
        _lib.check(_lib.lib().tkspmv_time_multi(self._h, ptr(dev_xs), int(n_x), int(iters), C.byref(ns)))
        return ns.value

    def debug_counters(self):
        """Checked thresholds of back-to-back queries (info()["batch_mode"]): how many selections failed their check so far (and
        sent their query through the repair launch), the suspension state of carried thresholds, batch launches so far."""
        out = (C.c_uint64 * 19)()
        _lib.check(_lib.lib().tkspmv_debug_counters(self._h, out, 19))
        return {"checks_failed": int(out[0]), "suspension_length": int(out[1]), "suspended_for": int(out[2]), "batch_launches": int(out[3]),
                "local_off_for_launches": int(out[4]), "local_off_length": int(out[5]),
                # tkspmv_run through the single-query kernel (local thresholds, checked): launches, queries repeated through the
                # exact launch because their check failed, and the suspension of carried thresholds that follows a failure
                "single_launches": int(out[6]), "single_repairs": int(out[7]), "single_checks_failed": int(out[8]),
                "single_suspended_for": int(out[9]),
                # batch launches that went out without a repair launch behind them (the host looks at their verdicts when it waits),
                # and the repairs that had to follow after all
                "trusted_launches": int(out[10]), "late_repairs": int(out[11]),
                # the pacing of back-to-back queries in force and what tkspmv_create's measurement of it took (0: static default)
                "pace_quantum": int(out[12]) & 0xFF, "pace_levels": (int(out[12]) >> 8) & 0xFF, "pace_base": (int(out[12]) >> 16) & 0xFF,
                "pace_period_ns": int(out[12]) >> 32,
                "pace_tuned_us": int(out[13]) & 0xFFFFFFFF, "pace_tune_launches": int(out[13]) >> 32,
                # option STATS, summed over the time_multi calls so far (the multi-query kernel's threshold exchange): queries, waves that
                # ran into their bounded wait for a threshold and the ticks (10 ns) they spent there, rows offered to / overflowed from the lists
                "multi_stat_queries": int(out[14]), "multi_waits": int(out[15]), "multi_wait_ticks": int(out[16]),
                "multi_rows_offered": int(out[17]), "multi_rows_overflowed": int(out[18])}

    def synchronize(self):
        _lib.check(_lib.lib().tkspmv_synchronize(self._h))

    def scores(self):
        """Full y = A.x of the current query (verification aid; the hot path never materialises it)."""
        y = np.empty(max(self.num_rows, 1), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_scores(self._h, f32p(y)))
        return y[:self.num_rows]

    def profile(self, dev_xs, n_x, iters):
        t = _lib.Timing()
        _lib.check(_lib.lib().tkspmv_profile(self._h, ptr(dev_xs), int(n_x), int(iters), C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_ if n != "reserved"}

    def result_device(self):
        a, b = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().tkspmv_result_device(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def info(self):
        """tkspmv_info as a dict. batch_compact / batch_packet_bytes / batch_stream_bytes: what the batch kernel streams -- 1280-byte
        packets re-encoded at 5 bytes per entry where the matrix's fp32 values share their top four bits (option F32_COMPACT), else
        the canonical stream that packed_bytes counts; the compact copies come on top of it, one per stream replica."""
        i = _lib.Info()
        _lib.check(_lib.lib().tkspmv_get_info(self._h, C.byref(i)))
        return i.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().tkspmv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextmanager
def _one_shot(m, **kw):
    """The engine of a one-shot helper: built for CooMatrix m with the helper's keywords, closed when the helper is done with it."""
    e = SpMV(m.row, m.col, m.val, m.rows, m.cols, **kw)
    try:
        yield e
    finally:
        e.close()


def topk_spmv(m, vec, k=100, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, run one query, return (values, indices). allow: a bool array of
    length m.rows (or row_mask() words): the top-k among those rows only (filtered query)."""
    with _one_shot(m, vec=vec, k=k, **kw) as e:
        if allow is not None:
            return e.run_filtered(allow=allow)
        e()
        return e.read_result()


def range_spmv(m, vec, threshold, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (values, indices) of every row scoring >= threshold (among the
    rows of `allow`, if given), sorted like topk_spmv's result."""
    kw.setdefault("k", 8)
    with _one_shot(m, vec=vec, **kw) as e:
        return e.run_range(threshold, allow=allow)


def facet_spmv(m, vec, threshold, groups, n_groups=None, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (counts, best_idx, best_val, total) of the rows scoring >=
    threshold (among the rows of `allow`, if given) per label groups[r] < n_groups (None: the largest label + 1): each label's
    matches, the row id and score of its best match ((0, 0.0) where it has none), and the number of all matches."""
    kw.setdefault("k", 8)
    with _one_shot(m, vec=vec, **kw) as e:
        e.set_groups(groups, n_groups)
        return e.run_facets(threshold, allow=allow)


def grouped_spmv(m, vec, groups, k=100, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (values, indices, groups) of the k best groups of rows (labels
    groups[r], one per row), each by its best row (among the rows of `allow`, if given), ordered like topk_spmv's result."""
    with _one_shot(m, vec=vec, k=k, **kw) as e:
        return e.run_grouped(allow=allow, groups=groups)


def ranked_spmv(m, vec, n, k=MAX_PAGE, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m with pages of k rows, return (values, indices) of the n best rows (among
    the rows of `allow`, if given) for ANY n, by search-after paging: ordered like topk_spmv's result, fewer than n when fewer
    rows are eligible."""
    with _one_shot(m, vec=vec, k=k, **kw) as e:
        vals, idxs, have = [], [], 0
        for v, i in e.pages(allow=allow):
            vals.append(v)
            idxs.append(i)
            have += i.size
            if have >= int(n):
                break
        if not vals:
            return np.empty(0, dtype=np.float32), np.empty(0, dtype=np.uint32)
        return np.concatenate(vals)[:int(n)], np.concatenate(idxs)[:int(n)]


def boosted_spmv(m, vec, k, weight=None, bias=None, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (values, indices) of the k rows (among the rows of `allow`, if
    given) with the best boosted scores weight[r] * score + bias[r] (either array may be None, not both), ordered like
    topk_spmv's result; values are boosted scores."""
    with _one_shot(m, vec=vec, k=k, **kw) as e:
        idx, val, n, _, _ = e.run_boosted(allow=allow, weight=weight, bias=bias)
        return val[:n], idx[:n]


def cosine_spmv(m, vec, k, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (values, indices) of the k rows (among the rows of `allow`, if
    given) with the largest cosine to vec, ordered like topk_spmv's result; values are cosines. vec is scaled to norm 1 (the norm
    in float64, every entry rounded once to float32; a zero vector stays zero) and the rows' weights come from set_cosine()."""
    v = np.asarray(vec, dtype=np.float64)
    norm = float(np.sqrt(np.sum(v * v)))
    x = (v / norm if norm > 0 else v).astype(np.float32)
    with _one_shot(m, vec=x, k=k, **kw) as e:
        e.set_cosine()
        idx, val, n, _, _ = e.run_boosted(allow=allow)
        return val[:n], idx[:n]


def boosted_range_spmv(m, vec, threshold, weight=None, bias=None, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (values, indices) of every row (among the rows of `allow`, if
    given) whose boosted score weight[r] * score + bias[r] is >= threshold (either array may be None, not both), sorted like
    topk_spmv's result; values are boosted scores."""
    kw.setdefault("k", 8)
    with _one_shot(m, vec=vec, **kw) as e:
        return e.run_boosted_range(threshold, allow=allow, weight=weight, bias=bias)


def boosted_facet_spmv(m, vec, threshold, groups, n_groups=None, weight=None, bias=None, allow=None, **kw):
    """One-shot helper: facet_spmv over boosted scores weight[r] * score + bias[r] (either array may be None, not both)."""
    kw.setdefault("k", 8)
    with _one_shot(m, vec=vec, **kw) as e:
        e.set_groups(groups, n_groups)
        return e.run_boosted_facets(threshold, allow=allow, weight=weight, bias=bias)


def boosted_grouped_spmv(m, vec, groups, k=100, weight=None, bias=None, allow=None, **kw):
    """One-shot helper: grouped_spmv over boosted scores weight[r] * score + bias[r] (either array may be None, not both)."""
    with _one_shot(m, vec=vec, k=k, **kw) as e:
        return e.run_boosted_grouped(allow=allow, groups=groups, weight=weight, bias=bias)


def cosine_range_spmv(m, vec, threshold, allow=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (values, indices) of every row (among the rows of `allow`, if
    given) whose cosine to vec is >= threshold, sorted like topk_spmv's result; values are cosines. vec is scaled to norm 1 as in
    cosine_spmv and the rows' weights come from set_cosine()."""
    v = np.asarray(vec, dtype=np.float64)
    norm = float(np.sqrt(np.sum(v * v)))
    x = (v / norm if norm > 0 else v).astype(np.float32)
    kw.setdefault("k", 8)
    with _one_shot(m, vec=x, **kw) as e:
        e.set_cosine()
        return e.run_boosted_range(threshold, allow=allow)


def assign_spmv(m, vecs, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (labels, best) of SpMV.assign(vecs): for every row the index of
    its best-scoring vector (ties to the smallest) and that score."""
    kw.setdefault("k", 8)
    with _one_shot(m, **kw) as e:
        return e.assign(vecs)


def nearest_spmv(m, vecs, n, mask=None, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (labels[rows, n], scores[rows, n]) of SpMV.nearest(vecs, n, mask):
    for every row (of the mask) its n best-scoring vectors in order and their scores."""
    kw.setdefault("k", 8)
    with _one_shot(m, **kw) as e:
        return e.nearest(vecs, n, mask)


def kmeans_spmv(m, cent, iters, **kw):
    """One-shot helper: build the engine for CooMatrix m, return (cent, labels, best) of SpMV.kmeans(cent, iters): spherical
    k-means whose assignment and centroid update both run on the device."""
    kw.setdefault("k", 8)
    with _one_shot(m, **kw) as e:
        return e.kmeans(cent, iters)


def knn_graph(m, k, rows=None, **kw):
    """The k-NN self-join (A.A^T top-n, what sparse_dot_topn computes on the CPU): for every row of CooMatrix m (or the given
    row ids) its k most similar OTHER rows, (values[n, k], indices[n, k]). The engine is built with k + 1 and the row itself
    is removed from its list."""
    k = int(k)
    if k < 1 or k + 1 > _lib.MAX_K:
        raise ValueError(f"k + 1 must be in [2, {_lib.MAX_K}]")
    first_row = int(kw.get("first_row", 0))
    ids = np.arange(first_row, first_row + m.rows, dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.uint32)
    with _one_shot(m, k=k + 1, **kw) as e:
        val, idx = e.similar(ids, exclude_self=True)
        return val[:, :k].copy(), idx[:, :k].copy()
