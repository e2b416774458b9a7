"""Boosted top-k (tkspmv_set_boost / tkspmv_enqueue_boosted / tkspmv_run_boosted) on the MI355X.

Every result is compared EXACTLY -- row ids, score bits, n, total, the next cursor -- with
    page_after(boost_scores(eng.scores(), w, b), present, k, cursor, min_score, first_row, allow)
(host.py): boost_scores is the numpy restatement of the transform, which tests/test_boost_host.py pins to a plain loop, page_after
the restatement of search-after paging, and eng.scores() the engine's own full score vector, which the older tests check. Device
outputs sit between guard zones. The conftest syncs torch only for the older enqueue names: these tests call
torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

import support
from support import GUARD, PageOut, bits_of, status_of

pytestmark = pytest.mark.gpu

START, AFTER, END = 0, 1, 2
NINF = float("-inf")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _same(got, want, what=""):
    idx, val, n, total, nxt = got
    ei, ev, en, et, ec = want
    assert (n, total) == (en, et), (what, n, total, en, et)
    assert np.array_equal(idx, ei), (what, "row ids differ from the expectation")
    assert np.array_equal(val.view(np.uint32), ev.view(np.uint32)), (what, "scores are not bit-identical")
    assert np.all(idx[en:] == 0) and np.all(val[en:].view(np.uint32) == 0), (what, "pads")
    assert nxt == ec, (what, nxt, ec)


def _dev(torch, a):
    """A float32 host array (or None) in device memory; keeps NaNs and signed zeros as they are."""
    return None if a is None else torch.from_numpy(_f32(a)).cuda()


def _query(eng, torch, dxs, count, w=None, b=None, stride=0, cursors=None, stream=0, after=False, **kw):
    """enqueue_boosted (w / b: device tensors or None; after: enqueue_after instead) into fresh guarded buffers; waits;
    [(idx, val, n, total, next)] per query."""
    out = PageOut(torch, count, eng.k)
    dcur = support.cursors(torch, cursors) if cursors is not None else None
    torch.cuda.synchronize()
    common = dict(dev_cursors=dcur.data_ptr() if dcur is not None else 0, stream=stream.cuda_stream if stream else 0, **out.ptrs(), **kw)
    if after:
        eng.enqueue_after(dxs.data_ptr() if dxs is not None else 0, count, **common)
    else:
        eng.enqueue_boosted(dxs.data_ptr() if dxs is not None else 0, count, w.data_ptr() if w is not None else 0,
                            b.data_ptr() if b is not None else 0, stride, **common)
    if stream:
        stream.synchronize()
    else:
        eng.synchronize()
    return out.read()


def _drop_rows(m, every, which):
    """The matrix without the entries of the rows r % every == which: rows without entries in the middle of the matrix."""
    keep = m.row % every != which
    m.row, m.col, m.val = m.row[keep].copy(), m.col[keep].copy(), m.val[keep].copy()
    return m


class _Setup:
    """One engine with its query installed, its own scores of that query and the presence flags the expectation pages over."""
    def __init__(self, pkg, torch, shape, k, dist="gamma", **kw):
        rows, cols, nnz = shape
        if "precision" in kw:
            kw["precision"] = getattr(pkg, kw["precision"])
        self.m = _drop_rows(pkg.generate_matrix(rows, cols, nnz, dist, rows % 97 + 5), 7, 3)
        self.x = pkg.create_sample_vector(cols, True, False, True, 19)
        self.rows, self.cols, self.k = rows, cols, k
        self.first_row, self.min_score = kw.get("first_row", 0), kw.get("min_score", 0.0)
        self.fp32 = "precision" not in kw
        self.eng = pkg.SpMV(self.m.row, self.m.col, self.m.val, rows, cols, k=k, device=0, **kw)
        self.eng.reset(self.x)
        self.y, self.present = self.eng.scores().copy(), support.present(self.m)
        self.dx = torch.from_numpy(self.x).cuda()

    def scores_of(self, x):
        """The engine's scores of another vector (the installed one is put back)."""
        self.eng.reset(x)
        y = self.eng.scores().copy()
        self.eng.reset(self.x)
        return y

    def expect(self, pkg, w=None, b=None, cursor=None, allow=None, y=None, k=None):
        t = pkg.boost_scores(self.y if y is None else y, w, b)
        return pkg.page_after(t, self.present, self.k if k is None else k, cursor, self.min_score, self.first_row, allow)

    def random_boost(self, seed):
        rng = np.random.default_rng(seed)
        return rng.uniform(0.5, 2.0, self.rows).astype(np.float32), rng.uniform(-1.0, 1.0, self.rows).astype(np.float32)


CONFIGS = {
    "tail": dict(shape=(2003, 512, 20), k=16),                      # rows % 4 == 3: the scalar tail
    "first_row": dict(shape=(20011, 1024, 20), k=100, first_row=5000),
    "c8": dict(shape=(20011, 1024, 20), k=100, nnz_per_lane=8),
    "f16": dict(shape=(20011, 1024, 20), k=100, precision="F16"),
    "fixed20": dict(shape=(20011, 1024, 20), k=100, precision="FIXED", fixed_width=20),
    "radix": dict(shape=(1000, 512, 20), k=100),                    # the engine that takes the radix route
    "tile_plus_one": dict(shape=(257, 64, 8), k=16, dist="uniform"),  # one tile of 256 rows plus one row
}


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request, pkg):
    import torch
    s = _Setup(pkg, torch, **CONFIGS[request.param])
    yield s
    s.eng.close()


@pytest.fixture(scope="module")
def tail(pkg):
    import torch
    s = _Setup(pkg, torch, **CONFIGS["tail"])
    yield s
    s.eng.close()


def test_random_weight_and_bias(pkg, setup):
    import torch
    s, eng = setup, setup.eng
    w, b = s.random_boost(1)
    dw, db = _dev(torch, w), _dev(torch, b)
    assert (~s.present).sum() > 0 and s.present.sum() > s.k
    for name, hw, hb, tw, tb in (("weight", w, None, dw, None), ("bias", None, b, None, db), ("both", w, b, dw, db)):
        top = s.expect(pkg, hw, hb)
        got, = _query(eng, torch, s.dx, 1, tw, tb)
        _same(got, top, name)
        assert got[2] == s.k and got[4][2] == AFTER
        # ... and the page behind it, and a page from the ranking's middle: the cursor's score_bits are boosted scores
        ranking = s.expect(pkg, hw, hb, k=s.rows)
        mid = ranking[2] // 2
        cursors = [top[4], (int(ranking[0][mid]), bits_of(ranking[1][mid]), AFTER), (17, bits_of(1e30), AFTER), (17, bits_of(1.0), END)]
        xs = torch.from_numpy(np.tile(s.x, (len(cursors), 1))).cuda()
        for c, g in zip(cursors, _query(eng, torch, xs, len(cursors), tw, tb, cursors=cursors)):
            _same(g, s.expect(pkg, hw, hb, c), (name, c))


def test_identities_are_enqueue_after_bit_for_bit(pkg, setup):
    import torch
    s, eng = setup, setup.eng
    plain = s.expect(pkg)
    cursors = [None, plain[4], (s.first_row + s.rows // 2, bits_of(np.median(s.y[s.present])), AFTER)]
    xs = torch.from_numpy(np.tile(s.x, (len(cursors), 1))).cuda()
    after = _query(eng, torch, xs, len(cursors), cursors=cursors, after=True)
    ones = _dev(torch, np.ones(s.rows, dtype=np.float32))
    nzero = _dev(torch, np.full(s.rows, -0.0, dtype=np.float32))
    assert np.all(nzero.cpu().numpy().view(np.uint32) == 0x80000000)
    for what, w, b in (("w = 1", ones, None), ("b = -0.0", None, nzero), ("w = 1, b = -0.0", ones, nzero)):
        got = _query(eng, torch, xs, len(cursors), w, b, cursors=cursors)
        for q in range(len(cursors)):
            _same(got[q], after[q], (what, q))
            _same(got[q], s.expect(pkg, None, None, cursors[q]), (what, q, "page_after"))


def test_ties(pkg, setup):
    import torch
    s, eng = setup, setup.eng
    zero = np.zeros(s.rows, dtype=np.float32)
    const = np.full(s.rows, 0.25, dtype=np.float32)
    got, = _query(eng, torch, s.dx, 1, _dev(torch, zero), _dev(torch, const))
    _same(got, s.expect(pkg, zero, const), "w = 0, b = 0.25")
    highest = np.flatnonzero(s.present)[::-1][:s.k] + s.first_row  # every present row ties: the highest ids, descending
    assert got[0].tolist() == highest.tolist() and np.all(got[1] == 0.25) and got[3] == int(s.present.sum())
    three = np.random.default_rng(6).choice(np.array([0.25, 0.5, 0.75], dtype=np.float32), s.rows)
    ranking = s.expect(pkg, zero, three, k=s.rows)
    cut = int((three[s.present] == 0.75).sum())  # the first row of the second tie class
    cursors = [None, (int(ranking[0][cut - 1]), bits_of(0.75), AFTER), (int(ranking[0][cut + 5]), bits_of(0.5), AFTER)]
    xs = torch.from_numpy(np.tile(s.x, (len(cursors), 1))).cuda()
    for c, g in zip(cursors, _query(eng, torch, xs, len(cursors), _dev(torch, zero), _dev(torch, three), cursors=cursors)):
        _same(g, s.expect(pkg, zero, three, c), ("three values", c))


def test_bottom_k_with_negated_scores(pkg):
    import torch
    s = _Setup(pkg, torch, (2003, 512, 20), 16, min_score=NINF)
    minus = np.full(s.rows, -1.0, dtype=np.float32)
    got, = _query(s.eng, torch, s.dx, 1, _dev(torch, minus))
    _same(got, s.expect(pkg, minus), "w = -1")
    lowest = np.sort(s.y[s.present])[:s.k]  # the bottom-k of the raw scores, negated
    assert np.array_equal(got[1].view(np.uint32), (-lowest).view(np.uint32)) and got[3] == int(s.present.sum())
    assert not np.any(~s.present[got[0]])  # a row without entries stays out even with min_score = -inf
    s.eng.close()


def test_overflow_and_nan_rows_never_appear(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    x = (s.x * np.float32(1024.0)).astype(np.float32)  # (scores large enough for 3e38 * score to overflow)
    y, dx = s.scores_of(x), torch.from_numpy(x).cuda()
    w, b = s.random_boost(2)
    best = s.expect(pkg, w, b, y=y)[0][:8].astype(np.int64)  # rows of the page's top: they would be returned
    w[best[:4]] = 3e38      # the product overflows
    b[best[4:8]] = np.nan   # a NaN bias, given through the device pointer
    with np.errstate(over="ignore"):
        assert np.all(y[best[:4]] * np.float32(3e38) == np.inf)
    want = s.expect(pkg, w, b, y=y, k=s.rows)
    assert not set(best.tolist()) & set(want[0][:want[2]].tolist())
    clean = s.expect(pkg, *s.random_boost(2), y=y)
    assert want[3] == clean[3] - 8  # not counted in total
    got, = _query(eng, torch, dx, 1, _dev(torch, w), _dev(torch, b))
    _same(got, s.expect(pkg, w, b, y=y), "overflow and NaN")
    assert not set(best.tolist()) & set(got[0].tolist())
    # ... and the scratch array holds no leftover of them: the same query without a boost is enqueue_after's
    _same(_query(eng, torch, s.dx, 1, after=True)[0], s.expect(pkg), "after, behind it")


def test_subnormal_products_and_sums(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    w = np.full(s.rows, 2.0 ** -130, dtype=np.float32)
    want = s.expect(pkg, w)
    assert want[2] == s.k and np.all(want[1][:s.k] > 0) and np.all(want[1][:s.k] < 2.0 ** -126), "the expected page must hold subnormal products"
    assert len(set(want[1][:s.k].tolist())) > s.k // 2  # (distinct subnormals: a flush to zero would order the page by row id)
    got, = _query(eng, torch, s.dx, 1, _dev(torch, w))
    _same(got, want, "subnormal products")
    b = np.full(s.rows, 2.0 ** -140, dtype=np.float32)
    got, = _query(eng, torch, s.dx, 1, _dev(torch, w), _dev(torch, b))
    _same(got, s.expect(pkg, w, b), "subnormal product + subnormal bias")


def test_min_score_applies_to_the_boosted_score(pkg):
    import torch
    probe = _Setup(pkg, torch, (2003, 512, 20), 16)
    ms = float(np.median(probe.y[probe.present]))
    probe.eng.close()
    s = _Setup(pkg, torch, (2003, 512, 20), 16, min_score=ms)
    assert np.array_equal(s.y.view(np.uint32), probe.y.view(np.uint32))
    above = s.present & (s.y >= np.float32(ms))
    b = np.where(above, -1000.0, 1000.0).astype(np.float32)  # pushes every eligible row under min_score and lifts every other one over it
    b[::5] = 0.0
    want = s.expect(pkg, None, b, k=s.rows)
    elig = set((want[0][:want[2]].astype(np.int64) - s.first_row).tolist())
    assert elig == set(np.flatnonzero(s.present & ((b == 1000.0) | ((b == 0.0) & above))).tolist())
    got, = _query(s.eng, torch, s.dx, 1, None, _dev(torch, b))
    _same(got, s.expect(pkg, None, b), "bias across min_score")
    assert got[3] == len(elig)
    s.eng.close()


def test_mask_with_boost(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    rng = np.random.default_rng(12)
    allow = rng.random(s.rows) < 0.5
    w, b = s.random_boost(3)
    masked = np.flatnonzero(s.present & ~allow)[:10]
    b[masked] = 1000.0  # a masked row with a large bias stays out
    dmask = torch.from_numpy(pkg.row_mask(s.rows, allow).view(np.int32)).cuda()
    want = s.expect(pkg, w, b, allow=allow)
    got, = _query(eng, torch, s.dx, 1, _dev(torch, w), _dev(torch, b), dev_mask=dmask.data_ptr())
    _same(got, want, "mask + boost")
    assert not set(masked.tolist()) & set(got[0].tolist())
    unmasked, = _query(eng, torch, s.dx, 1, _dev(torch, w), _dev(torch, b))
    assert set(masked.tolist()) <= set(unmasked[0].tolist())  # (without the mask they lead the page)
    got, = _query(eng, torch, s.dx, 1, _dev(torch, w), _dev(torch, b), cursors=[want[4]], dev_mask=dmask.data_ptr())
    _same(got, s.expect(pkg, w, b, want[4], allow), "mask + boost, page 2")


def test_full_walk_with_one_cursor_buffer(pkg, tail):
    import torch
    s, eng, k = tail, tail.eng, tail.k
    w, b = s.random_boost(4)
    dw, db = _dev(torch, w), _dev(torch, b)
    ranking = s.expect(pkg, w, b, k=s.rows)
    eligible = ranking[2]
    assert eligible % k != 0 and eligible > 20 * k
    pages = -(-eligible // k)
    out = PageOut(torch, pages, k)
    cur = support.cursors(torch, [None])
    torch.cuda.synchronize()
    for p in range(pages):  # all enqueued before the first wait, dev_next == dev_cursors
        ptrs = out.ptrs(p)
        ptrs["dev_next"] = cur.data_ptr()
        eng.enqueue_boosted(s.dx.data_ptr(), 1, dw.data_ptr(), db.data_ptr(), 0, dev_cursors=cur.data_ptr(), **ptrs)
    eng.synchronize()
    out.dev["dev_next"][GUARD:GUARD + 4 * pages] = 0  # (next went to the cursor buffer instead: read() checks the reserved words)
    got = out.read()
    left = eligible
    for p, (idx, val, n, total, _) in enumerate(got):
        assert (n, total) == (min(k, left), left), (p, n, total, left)
        lo = eligible - left
        assert np.array_equal(idx[:n], ranking[0][lo:lo + n]), (p, "row ids")
        assert np.array_equal(val[:n].view(np.uint32), ranking[1][lo:lo + n].view(np.uint32)), (p, "score bits")
        assert np.all(idx[n:] == 0) and np.all(val[n:].view(np.uint32) == 0), (p, "pads")
        left -= n
    assert left == 0
    assert cur.cpu().numpy().view(np.uint32).tolist() == [[0, 0, END, 0]], "the walk must end as END within ceil(eligible / k) calls"
    # the same walk through the host form
    walked = list(eng.boosted_pages(weight=w, bias=b))
    assert len(walked) == pages and all(v.size == k for v, _ in walked[:-1]) and 0 < walked[-1][0].size < k
    assert np.array_equal(np.concatenate([i for _, i in walked]), ranking[0][:eligible])
    assert np.array_equal(np.concatenate([v for v, _ in walked]).view(np.uint32), ranking[1][:eligible].view(np.uint32))
    eng.set_boost(None, None)


def test_four_queries_with_per_query_bias_and_unaligned_stride(pkg, tail):
    import torch
    s, eng, rows = tail, tail.eng, tail.rows
    rng = np.random.default_rng(14)
    xs = np.stack([pkg.create_sample_vector(s.cols, True, False, True, 40 + i) for i in range(4)]).astype(np.float32)
    ys = [s.scores_of(xs[q]) for q in range(4)]
    stride = rows + 3  # query 1 and 3 start 8 bytes off a multiple of 16: the scalar loads; query 0 and 2 the 16-byte loads
    assert (stride * 4) % 16 != 0 and (2 * stride * 4) % 16 == 0
    w = np.full((4, stride), np.nan, dtype=np.float32)  # (the three floats between two queries' arrays are never read)
    b = np.full((4, stride), np.nan, dtype=np.float32)
    w[:, :rows] = rng.uniform(0.5, 2.0, (4, rows))
    b[:, :rows] = rng.uniform(-1.0, 1.0, (4, rows))
    dxs, dw, db = torch.from_numpy(xs).cuda(), _dev(torch, w.ravel()), _dev(torch, b.ravel())
    assert dw.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    cursors = [None] + [s.expect(pkg, w[q, :rows], b[q, :rows], y=ys[q])[4] for q in range(1, 4)]
    got = _query(eng, torch, dxs, 4, dw, db, stride, cursors=cursors)
    for q in range(4):
        _same(got[q], s.expect(pkg, w[q, :rows], b[q, :rows], cursors[q], y=ys[q]), f"stride {stride}, query {q}")
    got = _query(eng, torch, dxs, 4, None, db, stride, cursors=cursors)  # the hybrid-fusion form: a per-query bias alone
    for q in range(4):
        _same(got[q], s.expect(pkg, None, b[q, :rows], cursors[q], y=ys[q]), f"bias alone, query {q}")
    got = _query(eng, torch, dxs, 4, dw, db, 0, cursors=cursors)  # stride 0: one pair for every query
    for q in range(4):
        _same(got[q], s.expect(pkg, w[0, :rows], b[0, :rows], cursors[q], y=ys[q]), f"stride 0, query {q}")
    # arrays that start off a multiple of 16 bytes
    off_w, off_b = _dev(torch, np.concatenate([[np.nan], w[2, :rows]])), _dev(torch, np.concatenate([[np.nan] * 3, b[2, :rows]]))
    out = PageOut(torch, 1, s.k)
    torch.cuda.synchronize()
    eng.enqueue_boosted(dxs.data_ptr(), 1, off_w.data_ptr() + 4, off_b.data_ptr() + 12, 0, **out.ptrs())
    eng.synchronize()
    _same(out.read()[0], s.expect(pkg, w[2, :rows], b[2, :rows], y=ys[0]), "unaligned pointers")


def test_installed_boost_run_boosted_and_a_callers_stream(pkg, tail):
    import torch
    s, eng, L = tail, tail.eng, pkg._lib
    w, b = s.random_boost(5)
    eng.set_boost(None, None)
    assert status_of(pkg, eng.enqueue_boosted, s.dx.data_ptr(), 1) == L.ERR_STATE  # both NULL, none installed
    assert status_of(pkg, eng.run_boosted) == L.ERR_STATE
    eng.set_boost(w, b)
    want = s.expect(pkg, w, b)
    _same(_query(eng, torch, s.dx, 1)[0], want, "both NULL: the installed boost")
    _same(_query(eng, torch, None, 1)[0], want, "the installed vector and the installed boost")
    _same(eng.run_boosted(), want, "run_boosted")
    rv, ri = eng.read_result()  # tkspmv_read sees the host form's page
    assert np.array_equal(ri, want[0]) and np.array_equal(rv.view(np.uint32), want[1].view(np.uint32))
    _same(eng.run_boosted(want[4]), s.expect(pkg, w, b, want[4]), "run_boosted, page 2")
    bad = w.copy()
    bad[100] = np.inf
    assert status_of(pkg, eng.set_boost, bad, b) == L.ERR_INVALID
    bad = b.copy()
    bad[s.rows - 1] = np.nan
    assert status_of(pkg, eng.set_boost, None, bad) == L.ERR_INVALID
    _same(eng.run_boosted(), want, "the boost installed before stays in force")
    with pytest.raises(ValueError):
        eng.set_boost(w[:-1])
    eng.set_boost(w)  # the weight alone: the bias installed before is gone
    _same(eng.run_boosted(), s.expect(pkg, w), "weight alone")
    eng.set_boost(bias=b)
    _same(eng.run_boosted(), s.expect(pkg, None, b), "bias alone")
    allow = np.random.default_rng(2).random(s.rows) < 0.3
    _same(eng.run_boosted(allow=allow, weight=w, bias=b), s.expect(pkg, w, b, allow=allow), "run_boosted with a mask")
    eng.set_filter(None)
    # a caller's stream, explicit arrays and the installed ones
    side = torch.cuda.Stream()
    dw, db = _dev(torch, w), _dev(torch, b)
    _same(_query(eng, torch, s.dx, 1, dw, db, stream=side)[0], want, "a caller's stream")
    _same(_query(eng, torch, s.dx, 1, stream=side)[0], want, "a caller's stream, installed boost")
    eng.set_boost(None, None)
    assert status_of(pkg, eng.run_boosted) == L.ERR_STATE
    val, idx = pkg.boosted_spmv(s.m, s.x, s.k, weight=w, bias=b)  # the one-shot helper
    assert np.array_equal(idx, want[0]) and np.array_equal(val.view(np.uint32), want[1].view(np.uint32))


def test_errors_in_the_stated_order(pkg):
    import torch
    L = pkg._lib
    m = pkg.generate_matrix(2003, 512, 20, "gamma", 4)
    x = pkg.create_sample_vector(512, True, False, True, 2)
    rows, k = m.rows, 16
    dmask = torch.from_numpy(pkg.row_mask(rows).view(np.int32)).cuda()
    dw = _dev(torch, np.ones(rows, dtype=np.float32))
    buf = torch.zeros(k, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    W = dw.data_ptr()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 512, k=k, device=0)
    assert status_of(pkg, eng.enqueue_boosted, 0, 1, W) == L.ERR_STATE     # no query vector installed
    assert status_of(pkg, eng.enqueue_boosted, 0, 1) == L.ERR_STATE        # ... and no boost either
    assert status_of(pkg, eng.run_boosted) == L.ERR_STATE
    assert status_of(pkg, eng.enqueue_boosted, 0, 2, W) == L.ERR_INVALID   # NULL dev_xs takes the installed vector: count must be 1
    assert status_of(pkg, eng.enqueue_boosted, 0, 2) == L.ERR_INVALID      # INVALID comes before STATE
    eng.reset(x)
    assert status_of(pkg, eng.enqueue_boosted, 0, 1) == L.ERR_STATE        # a vector, but no boost installed
    assert status_of(pkg, eng.enqueue_boosted, 0, 0, W) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_boosted, 0, -3, W) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_boosted, 0, 1, W, 0, -1) == L.ERR_INVALID  # a negative boost stride
    assert status_of(pkg, eng.enqueue_boosted, 0, 1, W, 0, 0, 0, dmask.data_ptr(), -1) == L.ERR_INVALID  # a negative mask stride
    for given in ((1, 0), (0, 1)):  # output pointers partly given
        p = [buf.data_ptr() if g else 0 for g in given]
        assert status_of(pkg, eng.enqueue_boosted, 0, 1, W, 0, 0, 0, 0, 0, *p) == L.ERR_INVALID
    n = C.c_int32(5)
    assert L.lib().tkspmv_run_boosted(eng._h, None, 1, None, None, C.byref(n), None, None) == L.ERR_INVALID  # use_filter, none installed
    assert n.value == 5
    idx, val, cnt, total, nxt = eng.run_boosted(weight=np.ones(rows, dtype=np.float32))  # ... and the engine still answers
    assert cnt == k and total > k and nxt[2] == AFTER
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 512, k=k, device=0, partitions=4, k_per_partition=8)  # the approximate per-partition path
    assert status_of(pkg, eng.enqueue_boosted, 0, 0, W) == L.ERR_INVALID      # INVALID comes first ...
    assert status_of(pkg, eng.enqueue_boosted, 0, 1) == L.ERR_UNSUPPORTED     # ... UNSUPPORTED before STATE (no vector, no boost)
    eng.reset(x)
    assert status_of(pkg, eng.enqueue_boosted, 0, 1, W) == L.ERR_UNSUPPORTED
    assert status_of(pkg, eng.run_boosted) == L.ERR_UNSUPPORTED
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 512, k=k, device=0, precision=pkg.F16)
    eng.reset(x)
    eng.run_boosted(weight=np.ones(rows, dtype=np.float32))  # served without a mask ...
    eng.set_boost(None, None)
    assert status_of(pkg, eng.enqueue_boosted, 0, 1, 0, 0, 0, 0, dmask.data_ptr()) == L.ERR_UNSUPPORTED  # ... a mask needs the filter kernels (before STATE)
    assert status_of(pkg, eng.enqueue_boosted, 0, 1, W, 0, 0, 0, dmask.data_ptr()) == L.ERR_UNSUPPORTED
    eng.close()


def test_engine_state_untouched(pkg):
    import torch
    s = _Setup(pkg, torch, (20011, 1024, 20), 100)
    eng, k, nq = s.eng, s.k, 8
    xs = np.stack([pkg.create_sample_vector(s.cols, True, False, True, 300 + i) for i in range(nq)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    w, b = s.random_boost(7)
    dw, db = _dev(torch, w), _dev(torch, b)
    ys = [s.scores_of(xs[q]) for q in range(3)]

    def batch():
        bi = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        bv = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.enqueue_batch(dxs.data_ptr(), nq, bi.data_ptr(), bv.data_ptr())
        eng.synchronize()
        return bi.cpu().numpy(), bv.cpu().numpy().view(np.uint32)

    first = batch()
    page = _query(eng, torch, s.dx, 1, cursors=[s.expect(pkg)[4]], after=True)[0]
    before = eng.debug_counters()
    got = _query(eng, torch, dxs, 3, dw, db)
    for q in range(3):
        _same(got[q], s.expect(pkg, w, b, y=ys[q]), f"query {q}")
    after = eng.debug_counters()
    assert after == before, (before, after)  # no batch or single launch, no check failed, nothing suspended
    again = batch()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    _same(_query(eng, torch, s.dx, 1, cursors=[s.expect(pkg)[4]], after=True)[0], page, "enqueue_after behind the boosted call")
    _same(page, s.expect(pkg, cursor=s.expect(pkg)[4]), "enqueue_after")
    s.eng.close()
