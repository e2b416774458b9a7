"""Range queries (tkspmv_enqueue_range / tkspmv_run_range) on the MI355X.

The expected match set of a query is { r : present[r] and allow[r] and yp[r] >= t } with yp, present from the order-matched
oracle (oracle.packed_scores of the engine's own layout), compared in fp32; the engine's output, as a set of (row, score bits)
pairs, must EQUAL it, and dev_counts must equal its size. Thresholds come from yp itself. The unfiltered cases with a finite
threshold above 0 are also checked against the independent gold leg (fp64 scores from the COO).
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import dataclasses

import numpy as np
import pytest

import support
from support import Scores, bits

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's north-star tolerance
BAND = 2e-6   # relative boundary band of the gold leg (test_gpu_filter.py's boundary tolerance)
FILL_I, FILL_V = 0xDEADBEEF, -7.0


def _engine(pkg, m, k, **kw):
    return pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, **kw)


def _expected(yp, present, allow, t, first_row=0):
    """{(first_row + r, bits(yp[r]))} of the rows that have entries, are allowed and score >= t, compared in fp32."""
    with np.errstate(invalid="ignore"):
        hit = present & allow & (yp.astype(np.float32) >= np.float32(t))
    rows = np.flatnonzero(hit)
    return set(zip((rows + first_row).tolist(), bits(yp[rows]).tolist()))


def _thresholds(yp, present, extra=()):
    """Scores at ranks 1, 10, ... (where the matrix has that many rows), fractions of the maximum, and one above the maximum."""
    s = np.sort(yp[present])[::-1]
    out = {f"rank{r}": float(s[r - 1]) for r in (1, 10, 100, 1000, 10_000, 100_000) if r <= s.size}
    mx = np.float32(s[0])
    for f in (0.9, 0.75, 0.5):
        out[f"{f}xmax"] = float(np.float32(f) * mx)
    out["above_max"] = float(np.nextafter(mx, np.float32(np.inf)))
    for name, v in extra:
        out[name] = v
    return out


class _Dev:
    """Device buffers of one enqueue_range call, filled with a known pattern."""
    def __init__(self, torch, nq, capacity):
        self.torch, self.nq, self.cap = torch, nq, capacity
        self.counts = torch.full((nq,), 12345, dtype=torch.int32, device="cuda")
        self.idx = torch.from_numpy(np.full((nq, max(capacity, 1)), FILL_I, dtype=np.uint32).view(np.int32)).cuda()
        self.val = torch.full((nq, max(capacity, 1)), FILL_V, dtype=torch.float32, device="cuda")

    def host(self):
        return (self.counts.cpu().numpy().view(np.uint32), self.idx.cpu().numpy().view(np.uint32), self.val.cpu().numpy())


def _check_query(count, idx, val, capacity, exp, label):
    """count: dev_counts[i]; idx / val: the query's capacity output entries."""
    assert int(count) == len(exp), f"{label}: dev_counts = {int(count)}, expected {len(exp)} matches"
    n = min(len(exp), capacity)
    got = list(zip(idx[:n].tolist(), bits(val[:n]).tolist()))
    assert len(set(r for r, _ in got)) == n, f"{label}: a row was returned twice"
    if len(exp) <= capacity:
        assert set(got) == exp, f"{label}: the match set differs from the order-matched oracle ({len(set(got) ^ exp)} pairs)"
    else:
        assert set(got) <= exp, f"{label}: a stored pair is no member of the expected set"
    assert np.all(idx[n:] == FILL_I) and np.all(bits(val[n:]) == bits(np.float32(FILL_V))), f"{label}: entries beyond min(count, capacity) were written"


def _gold_leg(oracle, m, x, t, got_rows, got_vals, first_row, label, y64_cache):
    if "y" not in y64_cache:
        y64_cache["y"] = oracle.scores_f64(m.row, m.col, m.val, x, m.rows)
    y64, p64 = y64_cache["y"]
    p64 = p64.astype(bool)
    band = p64 & (np.abs(y64 - t) <= BAND * abs(t))
    n_band = int(band.sum())
    print(f"{label}: t = {t!r}, {len(got_rows)} matches, {n_band} rows in the gold leg's band")
    assert n_band <= 16, f"{label}: {n_band} rows within {BAND} of the threshold"
    member = np.zeros(m.rows, dtype=bool)
    member[np.asarray(got_rows, dtype=np.int64) - first_row] = True
    gold = p64 & (y64 >= t)
    bad = np.flatnonzero((member != gold) & ~band)
    assert bad.size == 0, f"{label}: membership differs from fp64 outside the band for rows {bad[:8]}"
    if len(got_rows):
        r = np.asarray(got_rows, dtype=np.int64) - first_row
        assert np.allclose(np.asarray(got_vals, dtype=np.float64), y64[r], rtol=RTOL, atol=0), f"{label}: scores differ from fp64"


SHAPES = [
    (1_000_000, 1024, 20, 100, {}),
    (200_000, 4096, 20, 100, {}),
    (30_000, 16384, 20, 100, {}),
    (1000, 512, 20, 100, {}),
    (200_000, 1024, 20, 100, {"nnz_per_lane": 8}),
    (100_000, 1024, 20, 100, {"first_row": 5000}),
]
IDS = ["1Mx1024", "200kx4096", "30kx16384", "1000x512", "c8", "first_row"]


@pytest.mark.parametrize("rows,cols,nnz,k,kw", SHAPES, ids=IDS)
def test_range_matches_oracle(pkg, oracle, request, rows, cols, nnz, k, kw):
    import torch
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", rows % 97 + 3)
    x = pkg.create_sample_vector(cols, True, False, True, 17)
    first_row = kw.get("first_row", 0)
    eng = _engine(pkg, m, k, **kw)
    yp, present = Scores(pkg, eng, m)(oracle, x)
    extra = [("zero", 0.0), ("minus_one", -1.0), ("minus_inf", float("-inf"))] if rows == 1000 else []
    thr = _thresholds(yp, present, extra)
    eng.reset(x)
    eng()
    _, ui = eng.read_result()
    masks = {"unfiltered": None}
    masks.update(support.masks(rows, ui, first_row, rows))
    names = list(thr)
    nq = len(names)
    tv = np.array([thr[n] for n in names], dtype=np.float32)
    dthr = torch.from_numpy(tv).cuda()
    dxs = torch.from_numpy(np.tile(np.ascontiguousarray(x, dtype=np.float32), (nq, 1))).cuda()
    y64_cache = {}
    for mname, allow in masks.items():
        a = np.ones(rows, dtype=bool) if allow is None else allow
        exps = [_expected(yp, present, a, t, first_row) for t in tv]
        cap = max(1, max(len(e) for e in exps))
        dev = _Dev(torch, nq, cap)
        dmask = None if allow is None else torch.from_numpy(pkg.row_mask(rows, allow).view(np.int32)).cuda()
        torch.cuda.synchronize()
        eng.enqueue_range(dxs.data_ptr(), nq, dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), cap,
                          dmask.data_ptr() if dmask is not None else 0, 0)
        eng.synchronize()
        counts, gi, gv = dev.host()
        for i, name in enumerate(names):
            label = f"{request.node.callspec.id}/{mname}/{name}"
            _check_query(counts[i], gi[i], gv[i], cap, exps[i], label)
            if name in ("minus_inf", "minus_one", "zero"):
                assert len(exps[i]) == int((present & a).sum())  # non-negative data: every row with entries
            if name == "above_max":
                assert counts[i] == 0
            t = float(tv[i])
            if allow is None and np.isfinite(t) and t > 0.0:
                n = int(counts[i])
                _gold_leg(oracle, m, x, t, gi[i][:n], gv[i][:n], first_row, label, y64_cache)
    # a NaN threshold matches nothing
    dev = _Dev(torch, 1, 4)
    dnan = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_range(dxs.data_ptr(), 1, dnan.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), 4)
    eng.synchronize()
    counts, gi, gv = dev.host()
    _check_query(counts[0], gi[0], gv[0], 4, set(), "nan")
    eng.close()


def test_signed_data(pkg, oracle):
    """Random signs on the values and on the query: partial sums are no lower bounds of their rows' sums any more -- the case that
    would expose a trigger that is not an upper bound of every finished row."""
    import torch
    rows, cols, k = 50_000, 1024, 100
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 31)
    rng = np.random.default_rng(8)
    m = dataclasses.replace(m, val=(m.val * rng.choice(np.float32([-1.0, 1.0]), m.val.shape[0])).astype(np.float32))
    x = (pkg.create_sample_vector(cols, True, False, True, 19) * rng.choice(np.float32([-1.0, 1.0]), cols)).astype(np.float32)
    eng = _engine(pkg, m, k)
    yp, present = Scores(pkg, eng, m)(oracle, x)
    assert (yp[present] < 0).sum() > rows // 10
    s = np.sort(yp[present])[::-1]
    tv = np.array([s[9], s[999], s[s.size * 3 // 4]], dtype=np.float32)
    assert tv[2] < 0
    allow = np.ones(rows, dtype=bool)
    exps = [_expected(yp, present, allow, t) for t in tv]
    cap = max(len(e) for e in exps)
    dev = _Dev(torch, 3, cap)
    dthr = torch.from_numpy(tv).cuda()
    dxs = torch.from_numpy(np.tile(x, (3, 1))).cuda()
    torch.cuda.synchronize()
    eng.enqueue_range(dxs.data_ptr(), 3, dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), cap)
    eng.synchronize()
    counts, gi, gv = dev.host()
    for i in range(3):
        _check_query(counts[i], gi[i], gv[i], cap, exps[i], f"signed/{i}")
    eng.close()


@pytest.fixture(scope="module")
def mid(pkg, oracle):
    rows, cols, k, nq = 200_000, 1024, 100, 40  # 40 queries: more than one launch's worth
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 12)
    eng = _engine(pkg, m, k)
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 300 + i) for i in range(nq)]).astype(np.float32)
    sc = Scores(pkg, eng, m)
    scores = [sc(oracle, xs[i]) for i in range(nq)]
    yield m, eng, xs, scores
    eng.close()


def test_capacity(pkg, oracle, mid):
    import torch
    m, eng, xs, scores = mid
    yp, present = scores[0]
    s = np.sort(yp[present])[::-1]
    tv = np.array([s[999], s[99], s[9]], dtype=np.float32)
    allow = np.ones(m.rows, dtype=bool)
    exps = [_expected(yp, present, allow, t) for t in tv]
    dthr = torch.from_numpy(tv).cuda()
    dxs = torch.from_numpy(np.tile(xs[0], (3, 1))).cuda()
    cap = 64  # smaller than 1000 and 100, larger than 10
    dev = _Dev(torch, 3, cap)
    torch.cuda.synchronize()
    eng.enqueue_range(dxs.data_ptr(), 3, dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), cap)
    eng.synchronize()
    counts, gi, gv = dev.host()
    assert len(exps[0]) > cap and len(exps[1]) > cap and len(exps[2]) < cap
    for i in range(3):
        _check_query(counts[i], gi[i], gv[i], cap, exps[i], f"capacity/{i}")
    # counts only
    dcounts = torch.full((3,), 999, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_range(dxs.data_ptr(), 3, dthr.data_ptr(), dcounts.data_ptr())
    eng.synchronize()
    assert dcounts.cpu().numpy().tolist() == [len(e) for e in exps]


def test_sequences(pkg, oracle, mid):
    import torch
    m, eng, xs, scores = mid
    rows, nq = m.rows, xs.shape[0]
    rng = np.random.default_rng(3)
    allows = [rng.random(rows) < (0.5 if i % 3 else 0.02) for i in range(nq)]
    words = np.stack([pkg.row_mask(rows, a) for a in allows])
    wpr = words.shape[1]
    # per-query thresholds: the score at a rank that changes from query to query
    ranks = [10, 100, 1000, 3, 30_000]
    tv = np.array([np.sort(scores[i][0][scores[i][1]])[::-1][ranks[i % len(ranks)] - 1] for i in range(nq)], dtype=np.float32)
    dxs = torch.from_numpy(xs).cuda()
    dmask = torch.from_numpy(words.view(np.int32)).cuda()
    dthr = torch.from_numpy(tv).cuda()
    ones = np.ones(rows, dtype=bool)

    def go(label, mask_of, **kw):
        exps = [_expected(*scores[i], mask_of(i), tv[i]) for i in range(nq)]
        cap = max(1, max(len(e) for e in exps))
        dev = _Dev(torch, nq, cap)
        torch.cuda.synchronize()
        eng.enqueue_range(dxs.data_ptr(), nq, dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), cap, **kw)
        if "stream" in kw:
            side.synchronize()
        else:
            eng.synchronize()
        counts, gi, gv = dev.host()
        for i in range(nq):
            _check_query(counts[i], gi[i], gv[i], cap, exps[i], f"{label}/{i}")

    go("per_query_masks", lambda i: allows[i], dev_mask=dmask.data_ptr(), mask_stride=wpr)
    side = torch.cuda.Stream()  # (handle 0 would mean the engine's own)
    go("stride0_callers_stream", lambda i: allows[0], dev_mask=dmask.data_ptr(), mask_stride=0, stream=side.cuda_stream)
    go("unfiltered", lambda i: ones)


def test_run_range(pkg, oracle, mid):
    m, eng, xs, scores = mid
    yp, present = scores[5]
    s = np.sort(yp[present])[::-1]
    ones = np.ones(m.rows, dtype=bool)
    allow = np.random.default_rng(21).random(m.rows) < 0.3

    def sorted_pairs(exp):
        idx = np.array([r for r, _ in exp], dtype=np.uint32)
        val = np.array([b for _, b in exp], dtype=np.uint32).view(np.float32)
        return oracle.sort_tuples(idx, val)

    for t in (float(s[99]), float(s[4999])):
        # capacity=None: count first, then exactly that many
        val, idx = eng.run_range(t, vec=xs[5])
        ei, ev = sorted_pairs(_expected(yp, present, ones, t))
        assert np.array_equal(idx, ei) and np.array_equal(bits(val), bits(ev))
        assert eng.last_range_count == ei.size
        val, idx = eng.run_range(t, allow=allow)
        ei, ev = sorted_pairs(_expected(yp, present, allow, t))
        assert np.array_equal(idx, ei) and np.array_equal(bits(val), bits(ev))
    # a capacity that is too small: the true count, and `capacity` distinct members of the expected set, sorted among themselves
    t = float(s[4999])
    exp = _expected(yp, present, allow, t)
    val, idx = eng.run_range(t, allow=allow, capacity=50)
    assert eng.last_range_count == len(exp) and len(exp) > 50 and idx.size == 50
    got = set(zip(idx.tolist(), bits(val).tolist()))
    assert len(got) == 50 and got <= exp
    si, sv = oracle.sort_tuples(idx, val)
    assert np.array_equal(idx, si) and np.array_equal(bits(val), bits(sv))
    # a capacity larger than the count: all of them
    val, idx = eng.run_range(float(s[9]), allow=allow, capacity=50)
    ei, ev = sorted_pairs(_expected(yp, present, allow, float(s[9])))
    assert np.array_equal(idx, ei) and np.array_equal(bits(val), bits(ev)) and eng.last_range_count == ei.size
    eng.set_filter(None)
    # the one-shot helper
    small = pkg.generate_matrix(1000, 512, 20, "gamma", 5)
    x = pkg.create_sample_vector(512, True, False, True, 6)
    val, idx = pkg.range_spmv(small, x, 0.0, device=0)
    y, p = oracle.scores_f64(small.row, small.col, small.val, x, small.rows)
    assert sorted(idx.tolist()) == np.flatnonzero(p).tolist()
    assert np.all(np.diff(val) <= 0)


def _sequence(pkg, eng, xs, dxs, ranged, torch):
    """test_gpu_filter.py's sequence with a range sequence in place of the filtered one: enqueue_batch, (range sequence),
    enqueue_batch, tkspmv_run, enqueue_multi: the results of the top-k steps."""
    k, nq = eng.k, 8
    res = {}
    out_i = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    if ranged is not None:  # (not waited for: the range sequence runs right behind the batch launch, in stream order)
        dthr, dmask, wpr, dev, _ = ranged
        eng.enqueue_range(dxs.data_ptr(), nq, dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), dev.cap,
                          dmask.data_ptr(), wpr)
    eng.synchronize()
    res["batch1"] = (out_i.cpu().numpy().view(np.uint32).copy(), out_v.cpu().numpy().copy())
    out_i.zero_()
    out_v.zero_()
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr() + 4 * 4 * xs.shape[1], nq, out_i.data_ptr(), out_v.data_ptr())  # queries 4 .. 11
    eng.synchronize()
    res["batch2"] = (out_i.cpu().numpy().view(np.uint32).copy(), out_v.cpu().numpy().copy())
    eng.reset(xs[3])
    if ranged is not None:
        eng.run_range(float(ranged[4]))
    eng()
    v, i = eng.read_result()
    res["run"] = (i.copy(), v.copy())
    eng.reset(xs[5])
    eng.enqueue_multi(0, 1)
    v, i = eng.read_result()
    res["multi"] = (i.copy(), v.copy())
    return res


def test_no_cross_talk(pkg, oracle):
    import torch
    rows, cols, k = 200_000, 1024, 100
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 77)
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 500 + i) for i in range(16)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    rng = np.random.default_rng(9)
    allows = [rng.random(rows) < 0.1 for _ in range(8)]
    words = np.stack([pkg.row_mask(rows, a) for a in allows])
    dmask = torch.from_numpy(words.view(np.int32)).cuda()
    eng = _engine(pkg, m, k, multi_q=4)
    scores, sc = {}, Scores(pkg, eng, m)

    def yp_of(i):
        if i not in scores:
            scores[i] = sc(oracle, xs[i])
        return scores[i]
    tv = np.array([np.sort(yp_of(q)[0][yp_of(q)[1] & allows[q]])[::-1][49] for q in range(8)], dtype=np.float32)
    dthr = torch.from_numpy(tv).cuda()
    dev = _Dev(torch, 8, 256)
    got = _sequence(pkg, eng, xs, dxs, (dthr, dmask, words.shape[1], dev, tv[3]), torch)
    counters = eng.debug_counters()
    eng.close()
    ref = _engine(pkg, m, k, multi_q=4)
    _sequence(pkg, ref, xs, dxs, None, torch)
    ref_counters = ref.debug_counters()
    ref.close()
    counts, gi, gv = dev.host()
    for q in range(8):
        _check_query(counts[q], gi[q], gv[q], 256, _expected(*yp_of(q), allows[q], tv[q]), f"cross_talk/{q}")
        ei, ev = oracle.select_topk(*yp_of(q), k)
        assert np.array_equal(got["batch1"][0][q], ei) and np.array_equal(bits(got["batch1"][1][q]), bits(ev))
        ei, ev = oracle.select_topk(*yp_of(4 + q), k)
        assert np.array_equal(got["batch2"][0][q], ei) and np.array_equal(bits(got["batch2"][1][q]), bits(ev))
    ei, ev = oracle.select_topk(*yp_of(3), k)
    assert np.array_equal(got["run"][0], ei) and np.array_equal(bits(got["run"][1]), bits(ev))
    # the multi-query pass sums in its own order (row per lane): the oracle's segmented scores, as smoke() checks it
    y, present = oracle.scores_f32_segmented(m.row, m.col, m.val, xs[5], m.rows)
    ei, ev = oracle.select_topk(y, present, k)
    assert np.array_equal(got["multi"][0], ei) and np.array_equal(bits(got["multi"][1]), bits(ev))
    # no repair the sequence without the range queries would not have run
    for key in ("checks_failed", "late_repairs", "single_repairs"):
        assert counters[key] <= ref_counters[key], (key, counters, ref_counters)


def test_errors(pkg):
    import torch
    m = pkg.generate_matrix(20_000, 1024, 20, "gamma", 4)
    x = pkg.create_sample_vector(1024, True, False, True, 2)
    dthr = torch.full((4,), 0.5, dtype=torch.float32, device="cuda")
    dcnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
    dbuf_i = torch.zeros((4, 16), dtype=torch.int32, device="cuda")
    dbuf_v = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    dxs = torch.from_numpy(np.tile(x, (4, 1))).cuda()
    torch.cuda.synchronize()
    T, N, I, V, X = dthr.data_ptr(), dcnt.data_ptr(), dbuf_i.data_ptr(), dbuf_v.data_ptr(), dxs.data_ptr()

    def status_of(fn):
        with pytest.raises(pkg.TkspmvError) as e:
            fn()
        return e.value.status

    for kw in (dict(precision=pkg.Q1_7), dict(partitions=4, k_per_partition=8)):
        eng = _engine(pkg, m, 100, **kw)
        eng.reset(x)
        assert status_of(lambda: eng.enqueue_range(0, 1, T, N)) == pkg._lib.ERR_UNSUPPORTED, kw
        assert status_of(lambda: eng.run_range(0.5)) == pkg._lib.ERR_UNSUPPORTED, kw
        eng.close()
    eng = _engine(pkg, m, 100)
    assert status_of(lambda: eng.enqueue_range(0, 1, T, N)) == pkg._lib.ERR_STATE  # no query vector installed
    assert status_of(lambda: eng.run_range(0.5, capacity=4)) == pkg._lib.ERR_STATE
    eng.reset(x)
    INV = pkg._lib.ERR_INVALID
    assert status_of(lambda: eng.enqueue_range(X, 0, T, N)) == INV                       # count < 1
    assert status_of(lambda: eng.enqueue_range(X, 1, 0, N)) == INV                       # no thresholds
    assert status_of(lambda: eng.enqueue_range(X, 1, T, 0)) == INV                       # no counts
    assert status_of(lambda: eng.enqueue_range(X, 1, T, N, mask_stride=-1)) == INV       # negative stride
    assert status_of(lambda: eng.enqueue_range(X, 1, T, N, I, 0, 16)) == INV             # idx without val
    assert status_of(lambda: eng.enqueue_range(X, 1, T, N, 0, V, 16)) == INV             # val without idx
    assert status_of(lambda: eng.enqueue_range(X, 1, T, N, 0, 0, 16)) == INV             # capacity without outputs
    assert status_of(lambda: eng.enqueue_range(X, 1, T, N, I, V, 0)) == INV              # outputs without capacity
    assert status_of(lambda: eng.enqueue_range(0, 2, T, N)) == INV                       # the installed vector: count must be 1
    lib = pkg._lib.lib()
    import ctypes as C
    cnt = C.c_uint64(0)
    assert lib.tkspmv_run_range(eng._h, 0.5, 1, None, None, 0, C.byref(cnt)) == INV      # use_filter, none installed
    assert lib.tkspmv_run_range(eng._h, 0.5, 0, None, None, 0, None) == INV              # no count
    assert lib.tkspmv_run_range(eng._h, 0.5, 0, None, None, 4, C.byref(cnt)) == INV      # capacity without outputs
    # and the valid forms of the same calls go through
    eng.enqueue_range(X, 4, T, N, I, V, 16)
    eng.enqueue_range(0, 1, T, N)
    eng.synchronize()
    eng.close()
