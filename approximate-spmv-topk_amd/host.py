"""Host-side helpers mirroring the reference's common layer, bound to the native implementations in libtkspmv.so.

  Options               <- src/common/utils/options.hpp:37-133
  read_mtx              <- src/common/utils/utils.hpp:474-520 (readMtx) + mmio.hpp
  create_sample_vector  <- src/common/utils/utils.hpp:234-267
  generate_matrix       <- src/resources/python/create_matrices.py:58-128 (distributions; own PRNG)
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass
class CooMatrix:
    rows: int
    cols: int
    row: np.ndarray  # uint32 [nnz], non-decreasing when produced by the generator / a row-major MTX file
    col: np.ndarray  # uint32 [nnz]
    val: np.ndarray  # float32 [nnz]
    num_rows_coo: int = 0
    index_base: int = 0
    symmetric: bool = False

    @property
    def nnz(self):
        return int(self.row.shape[0])


def _coo_from_c(c):
    n = int(c.nnz)
    out = CooMatrix(
        rows=int(c.rows), cols=int(c.cols),
        row=np.ctypeslib.as_array(c.row, shape=(max(n, 1),))[:n].copy(),
        col=np.ctypeslib.as_array(c.col, shape=(max(n, 1),))[:n].copy(),
        val=np.ctypeslib.as_array(c.val, shape=(max(n, 1),))[:n].copy(),
        num_rows_coo=int(c.num_rows_coo), index_base=int(c.index_base), symmetric=bool(c.symmetric))
    _lib.lib().tkspmv_mtx_free(C.byref(c))
    return out


def read_mtx(path, index_base=0, read_values=True, sort=False):
    """readMtx(fname, ..., directed=0, read_values, debug, zero_indexed_file, sort_tuples).

    index_base=0 is the reference's compiled-in behaviour (zero_indexed_file=true at every call site);
    1 reads generator output (create_matrices.py writes 1-based ids); -1 auto-detects.
    Raises TkspmvError(ERR_IO) where the reference prints a message and exit(1)s.
    """
    c = _lib.Coo()
    _lib.check(_lib.lib().tkspmv_mtx_read(str(path).encode(), index_base, int(bool(read_values)), int(bool(sort)),
                                          C.byref(c)))
    return _coo_from_c(c)


def write_mtx(path, m, index_base=1, precision=10):
    row = np.ascontiguousarray(m.row, dtype=np.uint32)
    col = np.ascontiguousarray(m.col, dtype=np.uint32)
    val = np.ascontiguousarray(m.val, dtype=np.float32)
    _lib.check(_lib.lib().tkspmv_mtx_write(str(path).encode(), m.rows, m.cols, row.shape[0], _lib.u32p(row), _lib.u32p(col), _lib.f32p(val),
                                           index_base, precision))


def create_sample_vector(size, random=False, sum_to_one=True, norm_one=False, seed=0):
    """Same argument order and defaults as the reference; seed == 0 draws from std::random_device."""
    vec = np.empty(size, dtype=np.float32)
    _lib.check(_lib.lib().tkspmv_sample_vector(_lib.f32p(vec), size, int(random), int(sum_to_one), int(norm_one), int(seed)))
    return vec


def row_mask(rows, allow=None, exclude=None):
    """Allow-mask of a filtered query (SpMV.enqueue_filtered / set_filter): ceil(rows/32) uint32 words, bit r & 31 of word
    r >> 5 set when local row r may be returned (LSB first: numpy's packbits(..., bitorder="little") viewed as <u4).
    allow: bool array of length rows (None: every row); exclude: row ids to clear afterwards."""
    rows = int(rows)
    if rows < 0:
        raise ValueError("rows must be non-negative")
    if allow is None:
        bits = np.ones(rows, dtype=bool)
    else:
        bits = np.asarray(allow)
        if bits.dtype != np.bool_:
            raise ValueError("allow must be a bool array")
        if bits.shape != (rows,):
            raise ValueError(f"allow has shape {bits.shape}, expected ({rows},)")
        bits = bits.copy()
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64).ravel()
        if ex.size and (ex.min() < 0 or ex.max() >= rows):
            raise ValueError("exclude holds a row id outside [0, rows)")
        bits[ex] = False
    words = max(1, (rows + 31) // 32)
    padded = np.zeros(words * 32, dtype=bool)
    padded[:rows] = bits
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def _allow_words(rows, allow):
    """The `allow` argument of the host-array calls (SpMV.run_filtered and the like, Packed.col_stats) as contiguous uint32 mask
    words: a bool array of length rows goes through row_mask(), anything else is taken as mask words. The callers check the length."""
    a = np.asarray(allow)
    return np.ascontiguousarray(row_mask(rows, a) if a.dtype == np.bool_ else a, dtype=np.uint32)


def _mask_words(rows, mask, what):
    """The mask of Packed.nearest / Packed.col_stats as the words the C call takes: None stays None (every row); else _allow_words,
    ceil(rows / 32) of them (at least one)."""
    if mask is None:
        return None
    words = _allow_words(rows, mask)
    if words.shape != (max(1, (rows + 31) // 32),):
        raise ValueError(f"{what} must be bool[rows] or ceil(rows / 32) mask words")
    return words


def _vectors(vecs, cols, what="vectors"):
    """The vectors of the assignment calls as contiguous float32 [count >= 1, cols]; one vector of cols is a set of one."""
    xs = np.ascontiguousarray(vecs, dtype=np.float32)
    xs = xs.reshape(1, -1) if xs.ndim == 1 else xs
    if xs.ndim != 2 or xs.shape[0] < 1 or xs.shape[1] != cols:
        raise ValueError(f"{what} must be [count >= 1, {cols}]")
    return xs


def _order_key(f):
    """Monotone float32 -> uint32, the engine's order_key."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def collapse_topk(scores, present, groups, k, min_score=0.0, first_row=0):
    """The contract of grouped top-k (SpMV.enqueue_grouped) restated in numpy, for CPU-side users and as the tests' expectation:
    from float32 scores[rows], present[rows] (the row is eligible apart from its score: it has entries and is allowed) and
    groups[rows], the k best groups, each by the eligible row that comes first in the engine's order. Returns (idx[k] uint32 =
    row + first_row, val[k] float32, grp[k] uint32, n): n real entries, then pads (0, 0.0, 0xFFFFFFFF), like the device call.
    Ordering and eligibility go by the engine's 64-bit key (order key of the score << 32 | row): a row is eligible when its order
    key is at least min_score's and its score is above -inf; a larger key comes first."""
    y = np.ascontiguousarray(scores, dtype=np.float32)
    g = np.asarray(groups).astype(np.int64)
    ok = np.asarray(present).astype(bool)
    if y.ndim != 1 or g.shape != y.shape or ok.shape != y.shape:
        raise ValueError("scores, present and groups must be 1-D arrays of one length")
    key = _order_key(y)
    ok = ok & (key >= _order_key(np.array([min_score], dtype=np.float32))[0]) & (y > -np.inf)
    rows = np.flatnonzero(ok)
    ckey = (key[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    order = np.argsort(ckey, kind="stable")[::-1]  # (keys are unique: they carry the row)
    rows = rows[order]
    _, first = np.unique(g[rows], return_index=True)  # each group's first row in that order: its representative
    reps = rows[np.sort(first)][:int(k)]
    n = int(reps.size)
    idx = np.zeros(int(k), dtype=np.uint32)
    val = np.zeros(int(k), dtype=np.float32)
    grp = np.full(int(k), 0xFFFFFFFF, dtype=np.uint32)
    idx[:n] = reps + int(first_row)
    val[:n] = y[reps]
    grp[:n] = g[reps]
    return idx, val, grp, n


def page_after(y, present, k, cursor=None, min_score=0.0, first_row=0, allow=None):
    """The contract of search-after paging (SpMV.enqueue_after) restated in numpy, for CPU-side users and as the tests' expectation:
    from float32 y[rows] and present[rows] (the row has entries; allow[rows], if given, restricts further) the first k eligible
    rows that rank strictly behind `cursor` in the engine's order. cursor: None (from the top) or (row, score_bits, state) as
    tkspmv_cursor holds them -- a GLOBAL row id, the score's bit pattern, state 0 = START, 1 = AFTER, anything else = END.
    Returns (idx[k] uint32 = row + first_row, val[k] float32, n, total, next): n real entries, then pads (0, 0.0); total = the
    eligible rows behind the cursor, the returned ones included; next = (row, score_bits, 1) of the last real entry when
    total > k, else (0, 0, 2). Ordering, eligibility and the cut go by the engine's 64-bit key (order key of the score << 32 |
    global row id) and nothing else: a row is eligible when its order key is at least min_score's and its score is above -inf; it
    ranks behind an AFTER cursor when its key is below the cursor's; a larger key comes first."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    ok = np.asarray(present).astype(bool)
    if y.ndim != 1 or ok.shape != y.shape:
        raise ValueError("y and present must be 1-D arrays of one length")
    if allow is not None:
        a = np.asarray(allow)
        if a.dtype != np.bool_ or a.shape != y.shape:
            raise ValueError("allow must be a bool array of y's length")
        ok = ok & a
    k = int(k)
    key = _order_key(y)
    ok = ok & (key >= _order_key(np.array([min_score], dtype=np.float32))[0]) & (y > -np.inf)
    rows = np.flatnonzero(ok)
    ckey = (key[rows].astype(np.uint64) << np.uint64(32)) | (rows.astype(np.uint64) + np.uint64(int(first_row)))
    if cursor is not None:
        c_row, c_bits, c_state = (int(v) for v in cursor)
        if c_state == 1:
            c_key = _order_key(np.array([c_bits], dtype=np.uint32).view(np.float32))[0]
            behind = ckey < ((np.uint64(c_key) << np.uint64(32)) | np.uint64(c_row & 0xFFFFFFFF))
        else:
            behind = np.full(rows.shape, c_state == 0)
        rows, ckey = rows[behind], ckey[behind]
    total = int(rows.size)
    page = rows[np.argsort(ckey, kind="stable")[::-1][:k]]  # (keys are unique: they carry the row)
    n = int(page.size)
    idx = np.zeros(k, dtype=np.uint32)
    val = np.zeros(k, dtype=np.float32)
    idx[:n] = page + int(first_row)
    val[:n] = y[page]
    nxt = (int(idx[n - 1]), int(val[n - 1:n].view(np.uint32)[0]), 1) if total > k else (0, 0, 2)
    return idx, val, n, total, nxt


def boost_scores(y, weight=None, bias=None):
    """The contract of boosted top-k (SpMV.enqueue_boosted) restated in numpy: from float32 y[rows] the boosted scores
    weight[r] * y[r] + bias[r] as two separately rounded float32 operations (either array may be None: no multiply / no add;
    subnormal products and sums are kept, as the device keeps them). An entry of -inf (a row without entries, a masked row) stays
    -inf whatever weight and bias say; a result that is not finite (NaN, +inf, -inf) becomes -inf: such a row is never eligible.
    The expected page of a boosted query is page_after(boost_scores(y, weight, bias), present, ...)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    if y.ndim != 1:
        raise ValueError("y must be a 1-D array")
    t = y.copy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for a, op in ((weight, np.multiply), (bias, np.add)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.shape != y.shape:
                    raise ValueError(f"weight and bias must have y's shape {y.shape}")
                t = op(t, a, dtype=np.float32)
    ninf = np.float32(-np.inf)
    return np.where((y == ninf) | ~np.isfinite(t), ninf, t).astype(np.float32)


def boosted_matches(y, present, threshold, weight=None, bias=None, allow=None, first_row=0):
    """The contract of boosted range queries (SpMV.enqueue_boosted_range) restated in numpy, for CPU-side users and as the tests'
    expectation: from float32 y[rows] and present[rows] (the row has entries; allow[rows], if given, restricts further) the rows
    whose boosted score s' = boost_scores(y, weight, bias) is above -inf and >= threshold, compared as float32 (-inf matches every
    such row, NaN none; min_score plays no part). Returns (idx uint32 = row + first_row, val float32 = s', count), sorted like
    run_range's result: score descending (compared as floats: -0.0 and +0.0 tie), then row id descending."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    ok = np.asarray(present).astype(bool)
    if y.ndim != 1 or ok.shape != y.shape:
        raise ValueError("y and present must be 1-D arrays of one length")
    if allow is not None:
        a = np.asarray(allow)
        if a.dtype != np.bool_ or a.shape != y.shape:
            raise ValueError("allow must be a bool array of y's length")
        ok = ok & a
    sb = boost_scores(np.where(ok, y, np.float32(-np.inf)), weight, bias)
    with np.errstate(invalid="ignore"):
        ok = ok & (sb > -np.inf) & (sb >= np.float32(threshold))
    rows = np.flatnonzero(ok)
    rows = rows[np.lexsort((rows, sb[rows]))[::-1]]
    return (rows + int(first_row)).astype(np.uint32), sb[rows], int(rows.size)


def cosine_weights(m):
    """Weights that turn the engine's dot products into cosines by row (SpMV.set_boost(weight=...) with a query of norm 1):
    1 / ||row r||_2 of CooMatrix m, the squares summed in float64 and the result rounded once to float32; 0.0 for a row without
    entries or of norm 0. The device recipe (SpMV.set_cosine, SpMV.row_stats(ROW_INV_L2)) sums in float32 in the engine's own
    order and can differ from this one in the last bits."""
    sq = np.zeros(int(m.rows), dtype=np.float64)
    np.add.at(sq, np.asarray(m.row, dtype=np.int64), np.asarray(m.val, dtype=np.float64) ** 2)
    w = np.zeros(int(m.rows), dtype=np.float64)
    np.divide(1.0, np.sqrt(sq), out=w, where=sq > 0)
    return w.astype(np.float32)


def inv_l2(l2sq):
    """The finish of the ROW_INV_L2 row statistic (SpMV.row_stats, Packed.row_stats) restated in numpy, for CPU-side users and as
    the tests' expectation: from float32 sums of squares the cosine weights float32(1) / sqrt(l2sq), two separately rounded
    float32 operations (subnormals kept); 0.0 where l2sq is 0, inf or NaN, so every weight is finite."""
    s = np.ascontiguousarray(l2sq, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        w = np.divide(np.float32(1), np.sqrt(s, dtype=np.float32), dtype=np.float32)
    return np.where((s > 0) & np.isfinite(s), w, np.float32(0)).astype(np.float32)


def nearest(scores):
    """The contract of assignment (SpMV.assign, Packed.assign) restated in numpy, for CPU-side users and as the tests' expectation:
    from float32 scores[count, rows] -- scores[q, r] what row r scores for vector q -- (labels uint32[rows], best float32[rows]):
    vector 0 first, a later vector only where its score is strictly greater, so ties go to the smallest index and -0.0 never
    replaces +0.0. NaN scores are outside the contract."""
    labels, best = nearest_n(scores, 1)  # (a stable sort's first entry: the first of the largest scores, -0.0 and +0.0 tying)
    return np.ascontiguousarray(labels[:, 0]), np.ascontiguousarray(best[:, 0])


def nearest_n(scores, n, mask=None):
    """The contract of nearest-n assignment (SpMV.nearest, Packed.nearest) restated in numpy, for CPU-side users and as the tests'
    expectation: from float32 scores[count, rows] -- scores[q, r] what row r scores for vector q -- (labels uint32[rows, n], scores
    float32[rows, n]): a stable sort of the vectors by descending score, so ties (-0.0 and +0.0 among them) go to the smaller
    index; entries j >= count are (NEAREST_NONE, -inf). mask: bool[rows]; a row it excludes is (NEAREST_NONE, -inf) throughout.
    NaN scores are outside the contract."""
    y = np.ascontiguousarray(scores, dtype=np.float32)
    n = int(n)
    if y.ndim != 2 or y.shape[0] < 1:
        raise ValueError("scores must be [count >= 1, rows]")
    if not 1 <= n <= _lib.NEAREST_MAX_N:
        raise ValueError(f"n must be 1 .. {_lib.NEAREST_MAX_N}")
    count, rows = y.shape
    labels = np.full((rows, n), _lib.NEAREST_NONE, dtype=np.uint32)
    out = np.full((rows, n), -np.inf, dtype=np.float32)
    m = min(n, count)
    order = np.argsort(-(y + np.float32(0)).T, axis=1, kind="stable")[:, :m]  # (+ 0: -0.0 becomes +0.0, so the two tie as keys too)
    labels[:, :m] = order
    out[:, :m] = np.take_along_axis(y.T, order, axis=1)
    if mask is not None:
        a = np.asarray(mask)
        if a.dtype != np.bool_ or a.shape != (rows,):
            raise ValueError(f"mask must be a bool array of shape ({rows},)")
        labels[~a] = _lib.NEAREST_NONE
        out[~a] = -np.inf
    return labels, out


def margin(scores_n):
    """s1 - s2 of every row of nearest-n scores[rows, n] (float32[rows]): how sure the row's first assignment is. +inf where there is
    no second entry (n = 1, or a single vector); NaN for a row outside the mask, which has no first either."""
    s = np.ascontiguousarray(scores_n, dtype=np.float32)
    if s.ndim != 2 or s.shape[1] < 1:
        raise ValueError("scores must be [rows, n >= 1]")
    if s.shape[1] < 2:
        return np.where(np.isneginf(s[:, 0]), np.float32(np.nan), np.float32(np.inf)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (s[:, 0] - s[:, 1]).astype(np.float32)


def facet_counts(scores, present, labels, n_bins, threshold, first_row=0, allow=None):
    """The contract of facet counts (SpMV.enqueue_facets) restated in numpy, for CPU-side users and as the tests' expectation:
    from float32 scores[rows], present[rows] (the row has entries; allow[rows], if given, restricts further) and labels[rows], the
    rows that match -- score >= threshold, compared as float32: -inf matches every present row, NaN none -- counted per label.
    Returns (counts uint32[n_bins], best_idx uint32[n_bins], best_val float32[n_bins], total): counts[b] = matches with label b;
    best_idx[b] / best_val[b] = row + first_row and score of the bin's match that comes first in the engine's order, the maximum
    of the 64-bit key (order key of the score << 32 | global row id), (0, 0.0) for an empty bin; total = all matches, those whose
    label is >= n_bins (they belong to no bin) included."""
    y = np.ascontiguousarray(scores, dtype=np.float32)
    g = np.asarray(labels).astype(np.int64)
    ok = np.asarray(present).astype(bool)
    if y.ndim != 1 or g.shape != y.shape or ok.shape != y.shape:
        raise ValueError("scores, present and labels must be 1-D arrays of one length")
    if allow is not None:
        a = np.asarray(allow)
        if a.dtype != np.bool_ or a.shape != y.shape:
            raise ValueError("allow must be a bool array of scores' length")
        ok = ok & a
    n_bins = int(n_bins)
    with np.errstate(invalid="ignore"):
        ok = ok & (y >= np.float32(threshold))
    total = int(np.count_nonzero(ok))
    rows = np.flatnonzero(ok & (g >= 0) & (g < n_bins))
    u = y[rows].view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)  # the engine's order_key
    ckey = (key.astype(np.uint64) << np.uint64(32)) | (rows.astype(np.uint64) + np.uint64(int(first_row)))
    counts = np.bincount(g[rows], minlength=n_bins).astype(np.uint32)
    bkey = np.zeros(n_bins, dtype=np.uint64)
    np.maximum.at(bkey, g[rows], ckey)
    hi = (bkey >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi).astype(np.uint32)  # order_key's inverse
    filled = counts != 0
    best_idx = np.where(filled, (bkey & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.uint32(0)).astype(np.uint32)
    best_val = np.where(filled, bits, np.uint32(0)).astype(np.uint32).view(np.float32)
    return counts, best_idx, best_val, total


def bool_query(cols, must=(), must_not=(), should=(), min_should=0):
    """A boolean predicate over the rows' own columns (SpMV.match / enqueue_match) from lists of terms. Every item of `must` and of
    `should` is a column or an iterable of columns ("any of these") and takes one of the 32 clause bits, in this order: must first,
    then should; all the columns of `must_not` share one further bit. A row matches when it has an entry in every must clause, in none
    of the must_not columns and in at least min_should of the should clauses.
    Returns (clauses uint32[cols], (must, must_not, should, min_should)): the clause table -- bit c of clauses[j] set when column j
    belongs to clause c -- and the predicate's four words. Raises ValueError beyond 32 clauses or for a column outside [0, cols)."""
    cols = int(cols)
    clauses = np.zeros(cols, dtype=np.uint32)
    words = [0, 0, 0]
    bit = 0

    def columns(item):
        c = np.asarray(list(item) if hasattr(item, "__iter__") else [item]).astype(np.int64).ravel()
        if c.size and (c.min() < 0 or c.max() >= cols):
            raise ValueError(f"a column outside [0, {cols})")
        return c

    def clause(cs, which):
        nonlocal bit
        if bit >= 32:
            raise ValueError("a predicate holds at most 32 clauses")
        clauses[cs] |= np.uint32(1 << bit)
        words[which] |= 1 << bit
        bit += 1

    for item in must:
        clause(columns(item), 0)
    for item in should:
        clause(columns(item), 2)
    banned = [columns(item) for item in must_not]
    if banned:
        clause(np.concatenate(banned), 1)
    if int(min_should) < 0:
        raise ValueError("min_should must be non-negative")
    return clauses, (words[0], words[1], words[2], int(min_should))


def match_rows(row, col, rows, clauses, pred, allow=None):
    """The contract of term predicates (SpMV.enqueue_match) restated in numpy, for CPU-side users and as the tests' expectation:
    from the COO's row[nnz] / col[nnz] alone (values play no part: an explicit zero is an entry), the clause table and the
    predicate (must, must_not, should, min_should), bool[rows]: row r matches when it has entries, allow[r] if given, and its word
    W(r) -- the OR of clauses[col] over its entries -- has (W & must) == must, (W & must_not) == 0 and
    popcount(W & should) >= min_should."""
    rows = int(rows)
    r = np.asarray(row).astype(np.int64).ravel()
    c = np.asarray(col).astype(np.int64).ravel()
    t = np.ascontiguousarray(clauses, dtype=np.uint32)
    if r.shape != c.shape:
        raise ValueError("row and col must have one length")
    if r.size and (r.min() < 0 or r.max() >= rows or c.min() < 0 or c.max() >= t.size):
        raise ValueError("an entry outside the matrix")
    must, must_not, should, min_should = (int(v) & 0xFFFFFFFF for v in pred)
    W = np.zeros(rows, dtype=np.uint32)
    has = np.zeros(rows, dtype=bool)
    if r.size:
        v = t[c]
        if np.any(r[1:] < r[:-1]):  # (any entry order is a COO: the rows' runs are formed here)
            order = np.argsort(r, kind="stable")
            r, v = r[order], v[order]
        starts = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1])))
        W[r[starts]] = np.bitwise_or.reduceat(v, starts)
        has[r[starts]] = True
    hits = W & np.uint32(should)
    pop = np.zeros(rows, dtype=np.int64)
    for b in range(32):
        pop += (hits >> np.uint32(b)) & np.uint32(1)
    ok = has & ((W & np.uint32(must)) == np.uint32(must)) & ((W & np.uint32(must_not)) == 0) & (pop >= min_should)
    if allow is not None:
        a = np.asarray(allow)
        if a.dtype != np.bool_ or a.shape != (rows,):
            raise ValueError(f"allow must be a bool array of shape ({rows},)")
        ok &= a
    return ok


def col_stats(m, kind, allow=None):
    """The contract of column statistics (SpMV.enqueue_col_stats) restated in numpy from the COO alone, for CPU-side users and as
    the tests' expectation: for CooMatrix m one word per column over the entries whose row allow[rows] (bool, if given) allows --
    kind _lib.COL_NNZ: uint32, the number of entries stored in the column (explicit zeros, negative values and a column repeated
    within a row all count; 0 for a column without one); COL_MAX / COL_MIN: float32, the largest / smallest value in the engine's
    total order of floats (order_key: -0.0 < +0.0), -inf / +inf for a column without an entry."""
    kind, cols, rows = int(kind), int(m.cols), int(m.rows)
    if kind not in (_lib.COL_NNZ, _lib.COL_MAX, _lib.COL_MIN):
        raise ValueError("kind must be COL_NNZ, COL_MAX or COL_MIN")
    c = np.asarray(m.col).astype(np.int64).ravel()
    v = np.ascontiguousarray(m.val, dtype=np.float32).ravel()
    if allow is not None:
        a = np.asarray(allow)
        if a.dtype != np.bool_ or a.shape != (rows,):
            raise ValueError(f"allow must be a bool array of shape ({rows},)")
        keep = a[np.asarray(m.row).astype(np.int64).ravel()]
        c, v = c[keep], v[keep]
    if kind == _lib.COL_NNZ:
        return np.bincount(c, minlength=cols).astype(np.uint32)
    negate = np.uint32(0x80000000 if kind == _lib.COL_MIN else 0)  # the smallest value is the largest of the negated ones
    u = v.view(np.uint32) ^ negate
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)  # the engine's order_key
    best = np.zeros(cols, dtype=np.uint32)  # (0: no entry -- the key of no finite or infinite float)
    np.maximum.at(best, c, key)
    bits = np.where(best & np.uint32(0x80000000), best & np.uint32(0x7FFFFFFF), ~best).astype(np.uint32)  # order_key's inverse
    bits = np.where(best == 0, np.uint32(0xFF800000), bits) ^ negate
    return bits.astype(np.uint32).view(np.float32)


def quantise(values, exp):
    """quantise(v, E) of label sums (SpMV.enqueue_label_sums) restated in numpy integers: float32 values as int64 multiples of
    2^exp. |v| = m * 2^x with m the 24-bit significand (a subnormal: no hidden bit, x = -149); s = x - exp; s >= 0: m << s;
    s < 0: m >> -s rounded to nearest, ties to even on the magnitude (a shift of 64 or more gives 0); the sign of v. Defined
    for finite values with s <= 38."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    e = (bits >> np.uint64(23)) & np.uint64(0xFF)
    m = (bits & np.uint64(0x7FFFFF)) | np.where(e != 0, np.uint64(0x800000), np.uint64(0))
    s = np.where(e != 0, e.astype(np.int64) - 150, np.int64(-149)) - np.int64(int(exp))
    left = m << np.clip(s, 0, 39).astype(np.uint64)
    t = np.clip(-s, 1, 63).astype(np.uint64)
    q = m >> t
    rem, half = m & ((np.uint64(1) << t) - np.uint64(1)), np.uint64(1) << (t - np.uint64(1))
    q = q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) != 0))).astype(np.uint64)
    mag = np.where(s >= 0, left, q).astype(np.int64)
    return np.where((bits >> np.uint64(31)) != 0, -mag, mag)


def sums_exponent(m):
    """The default exponent of label sums for CooMatrix m (SpMV.sums_exponent): xmax + 1 + ceil_log2(max(1, the fullest column's
    entries)) - 62 with xmax the unbiased exponent of the largest |value| (-126 for a subnormal or zero); 0 without entries. No
    sum can reach 2^63 with it."""
    v = np.ascontiguousarray(m.val, dtype=np.float32).ravel()
    if v.size == 0:
        return 0
    e = int(np.max(v.view(np.uint32) & np.uint32(0x7FFFFFFF))) >> 23
    n = int(np.max(np.bincount(np.asarray(m.col).astype(np.int64).ravel())))
    return (e - 127 if e else -126) + 1 + (n - 1).bit_length() - 62


def label_sums(m, labels, n_bins, exp):
    """The contract of label sums (SpMV.enqueue_label_sums) restated in numpy from the COO alone, for CPU-side users and as the
    tests' expectation: int64 sums[n_bins, cols], sums[b, c] = the sum of quantise(v, exp) over the entries (r, c, v) of CooMatrix
    m with labels[r] == b. Every stored entry counts (explicit zeros, a column repeated within a row); a label >= n_bins has no
    bin."""
    n_bins, cols = int(n_bins), int(m.cols)
    lab = np.asarray(labels).astype(np.int64).ravel()
    if lab.shape != (int(m.rows),):
        raise ValueError(f"labels must have shape ({int(m.rows)},)")
    r = np.asarray(m.row).astype(np.int64).ravel()
    c = np.asarray(m.col).astype(np.int64).ravel()
    q = quantise(np.ascontiguousarray(m.val, dtype=np.float32).ravel(), exp)
    keep = lab[r] < n_bins
    sums = np.zeros(n_bins * cols, dtype=np.int64)
    np.add.at(sums, lab[r][keep] * cols + c[keep], q[keep])
    return sums.reshape(n_bins, cols)


def close_sums(sums, exp, mode, out=None):
    """The closing rules of label sums (SpMV.enqueue_sums_close) restated in numpy: from int64 sums[n_bins, cols] float32
    [n_bins, cols]. mode _lib.SUMS_FLOAT: ldexp(float32(sums), exp), the conversion rounding to nearest even. SUMS_UNIT: those
    values times inv_l2(float32(n2)), n2 the float64 sum of their squares taken as 64 partials (partial l: the columns l, l + 64,
    ... ascending) added in the order 0 .. 63; a bin whose weight is 0 keeps its row of `out` (zeros without one)."""
    s = np.ascontiguousarray(sums, dtype=np.int64)
    if s.ndim != 2 or int(mode) not in (_lib.SUMS_FLOAT, _lib.SUMS_UNIT):
        raise ValueError("sums must be [n_bins, cols] and mode SUMS_FLOAT or SUMS_UNIT")
    with np.errstate(over="ignore", under="ignore"):
        f = np.ldexp(s.astype(np.float32), np.int32(int(exp))).astype(np.float32)
    if int(mode) == _lib.SUMS_FLOAT:
        return f
    res = np.zeros_like(f) if out is None else np.array(out, dtype=np.float32).reshape(f.shape)
    sq = np.zeros((s.shape[0], (s.shape[1] + 63) // 64 * 64), dtype=np.float64)
    sq[:, :s.shape[1]] = f.astype(np.float64) ** 2
    part = np.zeros((s.shape[0], 64), dtype=np.float64)
    for k in range(sq.shape[1] // 64):
        part += sq[:, 64 * k:64 * k + 64]
    n2 = np.zeros(s.shape[0], dtype=np.float64)
    for lane in range(64):
        n2 += part[:, lane]
    with np.errstate(over="ignore"):
        w = inv_l2(n2.astype(np.float32))
    res[w != 0] = (f * w[:, None])[w != 0]
    return res


def idf_weights(df, n_rows, scheme="bm25"):
    """Inverse document frequency weights from document frequencies df[cols] (col_stats(COL_NNZ) of a matrix without repeated
    columns) and the number of rows n: scheme "bm25" is log(1 + (n - df + 0.5) / (df + 0.5)), "smooth" is log((1 + n) / (1 + df)) + 1;
    computed in float64, returned as float32, finite for df = 0."""
    d = np.asarray(df, dtype=np.float64)
    n = float(n_rows)
    if scheme == "bm25":
        w = np.log1p((n - d + 0.5) / (d + 0.5))
    elif scheme == "smooth":
        w = np.log((1.0 + n) / (1.0 + d)) + 1.0
    else:
        raise ValueError('scheme must be "bm25" or "smooth"')
    return w.astype(np.float32)


def score_bound(x, cmax, cmin):
    """An upper bound of every row's score x . row from the columns' extremes (col_stats COL_MAX / COL_MIN): the sum over the
    columns of max(0, x[c] * cmax[c], x[c] * cmin[c]) in float64; a column without entries (cmax = -inf) contributes 0. Holds for
    matrices whose rows do not repeat a column."""
    xv = np.asarray(x, dtype=np.float64)
    hi, lo = np.asarray(cmax, dtype=np.float64), np.asarray(cmin, dtype=np.float64)
    used = np.isfinite(hi) & np.isfinite(lo)
    hi, lo = np.where(used, hi, 0.0), np.where(used, lo, 0.0)
    return float(np.sum(np.maximum(0.0, np.maximum(xv * hi, xv * lo))))


def generate_matrix(rows, cols, avg_nnz, distribution="gamma", seed=1):
    dist = {"uniform": 0, "gamma": 1}[distribution]
    c = _lib.Coo()
    _lib.check(_lib.lib().tkspmv_generate(rows, cols, avg_nnz, dist, seed, C.byref(c)))
    return _coo_from_c(c)


def generate_matrix_rows(row_begin, row_end, cols, avg_nnz, distribution="gamma", seed=1):
    """Rows [row_begin, row_end) of generate_matrix(rows >= row_end, ...) with LOCAL row ids: a rank's shard of a
    row-sharded job, built without the whole matrix ever existing in the process."""
    dist = {"uniform": 0, "gamma": 1}[distribution]
    c = _lib.Coo()
    _lib.check(_lib.lib().tkspmv_generate_rows(row_begin, row_end, cols, avg_nnz, dist, seed, C.byref(c)))
    return _coo_from_c(c)


def generate_degrees(row_begin, row_end, avg_nnz, distribution="gamma", seed=1):
    """Row lengths of rows [row_begin, row_end) of the generated matrix (uint32 array)."""
    dist = {"uniform": 0, "gamma": 1}[distribution]
    deg = np.empty(max(row_end - row_begin, 1), dtype=np.uint32)
    _lib.check(_lib.lib().tkspmv_generate_degrees(row_begin, row_end, avg_nnz, dist, seed, _lib.u32p(deg)))
    return deg[:row_end - row_begin]


@dataclass
class Options:
    matrix_path: str
    use_sample_matrix: bool
    reset: bool
    num_tests: int
    debug: int
    ignore_matrix_values: bool
    top_k_value: int
    xclbin_path: str
    gpu_impl: int
    use_half_precision_gpu: bool
    block_size_1d: int
    block_size_2d: int
    num_blocks: int

    @staticmethod
    def parse(argv):
        """argv includes the program name, like main(argc, argv)."""
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        o = _lib.OptionsC()
        _lib.check(_lib.lib().tkspmv_options_parse(len(argv), arr, C.byref(o)))
        return Options(o.matrix_path.decode(), bool(o.use_sample_matrix), bool(o.reset), o.num_tests, o.debug,
                       bool(o.ignore_matrix_values), o.top_k_value, o.xclbin_path.decode(), o.gpu_impl,
                       bool(o.use_half_precision_gpu), o.block_size_1d, o.block_size_2d, o.num_blocks)


def sell_roundtrip(m, n_wave_partitions=4088, precision=_lib.F32):
    """Packs m into the wave-sliced ELL layout of the multi-query kernel and decodes it again (layout tests):
    (row, col, val, info) with the entries grouped by row, rows in stream order; info = dict of the layout's sizes."""
    row = np.ascontiguousarray(m.row, dtype=np.uint32)
    col = np.ascontiguousarray(m.col, dtype=np.uint32)
    val = np.ascontiguousarray(m.val, dtype=np.float32)
    d = _lib.Desc()
    d.rows, d.cols, d.nnz = m.rows, m.cols, row.shape[0]
    d.precision = int(precision)  # Q1_7_F32: byte chunks (Q1.7 rounded to nearest; decoded values are the rounded ones)
    d.row, d.col, d.val = _lib.u32p(row), _lib.u32p(col), _lib.f32p(val)
    nn = max(int(d.nnz), 1)
    orow, ocol, oval = np.empty(nn, np.uint32), np.empty(nn, np.uint32), np.empty(nn, np.float32)
    n = C.c_uint64()
    info = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().tkspmv_sell_roundtrip(C.byref(d), int(n_wave_partitions), _lib.u32p(orow), _lib.u32p(ocol), _lib.f32p(oval), C.byref(n), info))
    n = int(n.value)
    keys = ("slices", "chunks", "padded_entries", "partitions", "stream_bytes", "most_chunks_per_partition")
    return orow[:n], ocol[:n], oval[:n], dict(zip(keys, (int(v) for v in info)))


def sell_pack_device_check(m, n_wave_partitions=4088, precision=_lib.F32, device=-1):
    """Packs m into the wave-sliced ELL layout on the host and with the device packer (needs a GPU) and compares the two
    byte for byte: dict(identical, stream_bytes, chunks, host_ms, plan_ms, upload_ms, fill_ms)."""
    row = np.ascontiguousarray(m.row, dtype=np.uint32)
    col = np.ascontiguousarray(m.col, dtype=np.uint32)
    val = np.ascontiguousarray(m.val, dtype=np.float32)
    d = _lib.Desc()
    d.rows, d.cols, d.nnz = m.rows, m.cols, row.shape[0]
    d.precision, d.device = int(precision), int(device)
    d.row, d.col, d.val = _lib.u32p(row), _lib.u32p(col), _lib.f32p(val)
    info = (C.c_uint64 * 3)()
    ms = (C.c_double * 4)()
    _lib.check(_lib.lib().tkspmv_sell_pack_device_check(C.byref(d), int(n_wave_partitions), info, ms))
    return {"identical": bool(info[0]), "stream_bytes": int(info[1]), "chunks": int(info[2]), "host_ms": ms[0],
            "plan_ms": ms[1], "upload_ms": ms[2], "fill_ms": ms[3]}


class Packed:
    """Host-side packed (wave-BSCSR) matrix, for layout tests: decode(pack(A)) == A."""

    def __init__(self, m, k=100, nnz_per_lane=0, n_wave_partitions=4096, precision=_lib.F32, fixed_width=0, on_device=False,
                 device=-1):
        """on_device=True: packed by the HIP kernels of csrc/device_pack.hip (needs a GPU) instead of the host packer; the
        result is copied back, so decode() / raw() / save() work alike. self.pack_ms = (upload, kernels) then."""
        self._h = C.c_void_p()
        self._row = np.ascontiguousarray(m.row, dtype=np.uint32)
        self._col = np.ascontiguousarray(m.col, dtype=np.uint32)
        self._val = np.ascontiguousarray(m.val, dtype=np.float32)
        d = _lib.Desc()
        d.rows, d.cols, d.nnz = m.rows, m.cols, self._row.shape[0]
        d.row, d.col, d.val = _lib.u32p(self._row), _lib.u32p(self._col), _lib.f32p(self._val)
        d.k, d.precision, d.nnz_per_lane, d.fixed_width = k, precision, nnz_per_lane, fixed_width
        d.device = device
        self.pack_ms = None
        if on_device:
            ms = (C.c_double * 2)()
            _lib.check(_lib.lib().tkspmv_pack_device(C.byref(d), n_wave_partitions, C.byref(self._h), ms))
            self.pack_ms = (ms[0], ms[1])
        else:
            _lib.check(_lib.lib().tkspmv_pack(C.byref(d), n_wave_partitions, C.byref(self._h)))
        self.nnz = int(d.nnz)

    @classmethod
    def load(cls, path):
        """A packed matrix read back from a .tkspmv file (raises TkspmvError ERR_IO if it is missing or damaged)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().tkspmv_packed_load(str(path).encode(), C.byref(self._h)))
        self.nnz = self.info()["nnz"]
        return self

    def save(self, path):
        _lib.check(_lib.lib().tkspmv_packed_save(self._h, str(path).encode()))

    @staticmethod
    def wave_partitions(device=-1, waves_per_cu=0, threads_per_wg=0, m=None, precision=_lib.F32, nnz_per_lane=0):
        """Wave partitions an engine on `device` cuts a matrix into (the n_wave_partitions to pack for). Needs a GPU. With the
        matrix `m` given: the hint tkspmv_create itself would use for it (small matrices keep 4 workgroups for selections);
        without: the largest count an engine of this geometry accepts."""
        d = _lib.Desc()
        d.device, d.waves_per_cu, d.threads_per_wg = int(device), int(waves_per_cu), int(threads_per_wg)
        if m is not None:
            d.rows, d.cols, d.nnz, d.precision, d.nnz_per_lane = int(m.rows), int(m.cols), int(m.row.shape[0]), int(precision), int(nnz_per_lane)
        n = C.c_uint32()
        _lib.check(_lib.lib().tkspmv_wave_partitions(C.byref(d), C.byref(n)))
        return int(n.value)

    def info(self):
        i = _lib.Info()
        _lib.check(_lib.lib().tkspmv_packed_info(self._h, C.byref(i)))
        return i.as_dict()

    def decode(self):
        row = np.empty(max(self.nnz, 1), dtype=np.uint32)
        col = np.empty(max(self.nnz, 1), dtype=np.uint32)
        val = np.empty(max(self.nnz, 1), dtype=np.float32)
        n = C.c_uint64()
        _lib.check(_lib.lib().tkspmv_packed_decode(self._h, _lib.u32p(row), _lib.u32p(col), _lib.f32p(val), C.byref(n)))
        n = int(n.value)
        return row[:n], col[:n], val[:n]

    def get_row(self, row):
        """(cols, vals) of one row, in stream order (= the order of the COO): found by bisecting the packets' row table, the lookup
        the engine's row_vectors_kernel runs on the device. fp32 values only (TkspmvError ERR_UNSUPPORTED otherwise)."""
        n = C.c_uint32()
        L = _lib.lib()
        _lib.check(L.tkspmv_packed_get_row(self._h, int(row), None, None, 0, C.byref(n)))
        col = np.empty(max(n.value, 1), dtype=np.uint32)
        val = np.empty(max(n.value, 1), dtype=np.float32)
        if n.value:
            _lib.check(L.tkspmv_packed_get_row(self._h, int(row), _lib.u32p(col), _lib.f32p(val), n.value, C.byref(n)))
        return col[:n.value], val[:n.value]

    def score_rows(self, x, rows):
        """float32 scores of the given LOCAL rows for the vector x, with the bits an engine created from this packed matrix reports
        (SpMV.score_rows, SpMV.scores): each row's own packets through the streaming kernels' arithmetic, on the host. A row without
        entries scores +0.0. fp32 values only (TkspmvError ERR_UNSUPPORTED otherwise); ERR_INVALID for a row >= rows."""
        ids = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        xv = np.ascontiguousarray(x, dtype=np.float32)
        if xv.shape != (self.info()["cols"],):
            raise ValueError(f"vector has shape {xv.shape}, expected ({self.info()['cols']},)")
        out = np.empty(ids.size, dtype=np.float32)
        if ids.size:
            _lib.check(_lib.lib().tkspmv_packed_score_rows(self._h, _lib.f32p(xv), _lib.u32p(ids), int(ids.size), _lib.f32p(out)))
        return out

    def row_stats(self, kind):
        """float32[rows]: one statistic of every row (kind: _lib.ROW_NNZ entries, ROW_L1 sum of |v|, ROW_L2SQ sum of v*v, ROW_INV_L2
        the cosine weight 1/sqrt(L2SQ), 0.0 where that sum is 0, inf or NaN), with the bits an engine created from this packed
        matrix reports (SpMV.row_stats): the sums are formed in the streaming kernels' order, on the host. A row without entries
        gives +0.0. fp32 values only (TkspmvError ERR_UNSUPPORTED otherwise); ERR_INVALID for a kind outside 0..3."""
        out = np.empty(max(int(self.info()["rows"]), 1), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_packed_row_stats(self._h, int(kind), _lib.f32p(out)))
        return out[:int(self.info()["rows"])]

    def assign(self, vecs):
        """(labels uint32[rows], best float32[rows]): for every row the index of the best-scoring of vecs[count, cols] (ties to the
        smallest) and that score, with the bits an engine created from this packed matrix reports (SpMV.assign): score_rows'
        arithmetic per row and vector, on the host. A row without entries gets label 0 and +0.0. fp32 values only (TkspmvError
        ERR_UNSUPPORTED otherwise)."""
        rows, cols = int(self.info()["rows"]), int(self.info()["cols"])
        xs = _vectors(vecs, cols)
        labels = np.empty(max(rows, 1), dtype=np.uint32)
        best = np.empty(max(rows, 1), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_packed_assign(self._h, _lib.f32p(xs), int(xs.shape[0]), _lib.u32p(labels), _lib.f32p(best)))
        return labels[:rows], best[:rows]

    def label_sums(self, labels, n_bins, exp, mode=_lib.SUMS_RAW, out=None):
        """(sums int64[n_bins, cols], floats float32[n_bins, cols] or None): the label sums of the packed matrix with the bits an
        engine created from it reports (SpMV.label_sums): every row located in the stream, quantise(v, exp) of its entries added
        to the word of labels[row] and their column; mode SUMS_FLOAT / SUMS_UNIT adds the closing rule (UNIT: a bin whose norm is
        0 or overflows keeps its row of `out`, zeros without one). fp32 values only (TkspmvError ERR_UNSUPPORTED otherwise)."""
        rows, cols = int(self.info()["rows"]), int(self.info()["cols"])
        lab = np.ascontiguousarray(labels, dtype=np.uint32).ravel()
        if lab.shape != (rows,):
            raise ValueError(f"labels must have shape ({rows},)")
        lab = lab if rows else np.zeros(1, dtype=np.uint32)
        n_bins = int(n_bins)
        sums = np.zeros((max(n_bins, 1), max(cols, 1)), dtype=np.int64)
        res = None
        if int(mode) != _lib.SUMS_RAW:
            res = np.zeros((n_bins, cols), dtype=np.float32) if out is None else np.array(out, dtype=np.float32).reshape(n_bins, cols)
        _lib.check(_lib.lib().tkspmv_packed_label_sums(self._h, _lib.u32p(lab), n_bins, int(exp), int(mode), _lib.i64p(sums), _lib.f32p(res)))
        return sums.reshape(-1)[:n_bins * cols].reshape(n_bins, cols), res

    def sums_exponent(self):
        """The default exponent of label sums (SpMV.sums_exponent) from the packed matrix's own column statistics."""
        e = C.c_int32()
        _lib.check(_lib.lib().tkspmv_packed_sums_exponent(self._h, C.byref(e)))
        return int(e.value)

    def nearest(self, vecs, n, mask=None):
        """(labels uint32[rows, n], scores float32[rows, n]): for every row its n best-scoring of vecs[count, cols] in order -- score
        descending, ties to the smaller index --, with the bits an engine created from this packed matrix reports (SpMV.nearest):
        score_rows' arithmetic per row and vector, on the host. Entries beyond count are (NEAREST_NONE, -inf); so is every entry of
        a row outside mask (a bool array of length rows, or row_mask() words; None: every row). 1 <= n <= NEAREST_MAX_N. fp32 values
        only (TkspmvError ERR_UNSUPPORTED otherwise)."""
        rows, cols = int(self.info()["rows"]), int(self.info()["cols"])
        xs, n, words = _vectors(vecs, cols), int(n), _mask_words(rows, mask, "mask")
        labels = np.empty((max(rows, 1), max(n, 1)), dtype=np.uint32)
        scores = np.empty((max(rows, 1), max(n, 1)), dtype=np.float32)
        _lib.check(_lib.lib().tkspmv_packed_nearest(self._h, _lib.f32p(xs), int(xs.shape[0]), n, _lib.u32p(words), _lib.u32p(labels), _lib.f32p(scores)))
        return labels[:rows], scores[:rows]

    def col_stats(self, kind, allow=None):
        """uint32[cols] (kind _lib.COL_NNZ) or float32[cols] (COL_MAX, COL_MIN): one statistic of every column over all rows, or over
        the rows allow (a bool array of length rows, or row_mask() words) allows, with the bits an engine created from this packed
        matrix reports (SpMV.col_stats): a walk over the packet stream, placeholders and padding dropped. fp32 values only
        (TkspmvError ERR_UNSUPPORTED otherwise); ERR_INVALID for a kind outside 0..2."""
        rows, cols = int(self.info()["rows"]), int(self.info()["cols"])
        words = _mask_words(rows, allow, "allow")
        out = np.empty(max(cols, 1), dtype=np.uint32)
        _lib.check(_lib.lib().tkspmv_packed_col_stats(self._h, int(kind), _lib.u32p(words), _lib.ptr(out.ctypes.data)))
        out = out[:cols]
        return out if int(kind) == _lib.COL_NNZ else out.view(np.float32)

    def raw(self):
        """(packets bytes, packet_bytes, pkt_row, part_first, part_count) as numpy views/copies."""
        pk = C.c_void_p()
        pb = C.c_uint64()
        prow = C.POINTER(C.c_uint32)()
        pf = C.POINTER(C.c_uint32)()
        pc = C.POINTER(C.c_uint32)()
        npart = C.c_uint32()
        _lib.check(_lib.lib().tkspmv_packed_raw(self._h, C.byref(pk), C.byref(pb), C.byref(prow), C.byref(pf),
                                                C.byref(pc), C.byref(npart)))
        info = self.info()
        n_packets, n_parts = info["n_packets"], int(npart.value)
        nbytes = n_packets * int(pb.value)
        packets = np.ctypeslib.as_array(C.cast(pk, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes].copy()
        pkt_row = np.ctypeslib.as_array(prow, shape=(max(n_packets, 1),))[:n_packets].copy()
        part_first = np.ctypeslib.as_array(pf, shape=(max(n_parts, 1),))[:n_parts].copy()
        part_count = np.ctypeslib.as_array(pc, shape=(max(n_parts, 1),))[:n_parts].copy()
        return packets, int(pb.value), pkt_row, part_first, part_count

    def close(self):
        if self._h:
            _lib.lib().tkspmv_packed_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
