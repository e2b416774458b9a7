"""Boosted range, facet and grouped queries (tkspmv_enqueue_boosted_range / _facets / _grouped and their run_* forms) on the MI355X.

Every result is compared EXACTLY with the contract's restatement on the order-matched oracle's scores y of the engine's own layout
(the engine's own full score vector for F16 and fixed point): with sb = boost_scores(y, w, b) and ok = present & allow & (sb > -inf),
    range:   boosted_matches(y, present, threshold, w, b, allow, first_row)   as a set of (row, score bits), and its count
    facets:  facet_counts(sb, ok, labels, n_bins, threshold, first_row)        element for element
    grouped: collapse_topk(sb, ok, groups, k, min_score, first_row)            element for element
Device outputs sit between guard zones. The conftest syncs torch only for the older enqueue names: these tests call
torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

import support
from support import EngineSetup, GuardedOut, bits, status_of

pytestmark = pytest.mark.gpu

NINF = float("-inf")
LDS_CAP = 4096  # bins of boosted_bins_kernel's histogram in LDS


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _dev(torch, a, dtype=np.float32):
    """A host array (or None) in device memory; keeps NaNs and signed zeros as they are."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).cuda()


def _p(t):
    return t.data_ptr() if t is not None else 0


class _Setup(EngineSetup):
    """EngineSetup on a matrix with a seventh of its rows emptied; `signs`: matrix and query carry random signs."""
    def __init__(self, pkg, oracle, torch, c):
        self.signs = c.get("signs", False)
        self.pkg, self.oracle = pkg, oracle
        super().__init__(pkg, oracle, torch, c)
        self.rows, self.cols = self.m.rows, self.m.cols
        if self.signs:
            self.x = (self.x * np.where(np.random.default_rng(8).random(self.cols) < 0.5, -1.0, 1.0)).astype(np.float32)
            self.y, self.present = self.scores(oracle, self.x)
            self.eng.reset(self.x)
            self.dx = torch.from_numpy(self.x).cuda()
        rng = np.random.default_rng(self.rows)
        self.labels = rng.integers(0, 7, self.rows).astype(np.uint32)
        self.eng.set_groups(self.labels, 7)

    def matrix(self, m):
        keep = m.row % 7 != 3
        m.row, m.col, m.val = m.row[keep].copy(), m.col[keep].copy(), m.val[keep].copy()
        return support.signed(self.pkg, m, 4) if self.signs else m

    def scores_of(self, x):
        """y of another vector: the oracle's for fp32 engines, else the engine's own (the installed vector is put back)."""
        if self.fp32:
            return self.scores(self.oracle, x)[0]
        self.eng.reset(x)
        y = self.eng.scores().copy()
        self.eng.reset(self.x)
        return y

    def random_boost(self, seed):
        rng = np.random.default_rng(seed)
        return rng.uniform(0.5, 2.0, self.rows).astype(np.float32), rng.uniform(-1.0, 1.0, self.rows).astype(np.float32)

    def sb_ok(self, w=None, b=None, allow=None, y=None):
        sb = self.pkg.boost_scores(self.y if y is None else y, w, b)
        ok = self.present & (sb > -np.inf)
        return sb, ok if allow is None else ok & allow

    def want_range(self, tau, w=None, b=None, allow=None, y=None):
        return self.pkg.boosted_matches(self.y if y is None else y, self.present, tau, w, b, allow, self.first_row)

    def want_facets(self, tau, w=None, b=None, allow=None, y=None, labels=None, n_bins=7):
        sb, ok = self.sb_ok(w, b, allow, y)
        return self.pkg.facet_counts(sb, ok, self.labels if labels is None else labels, n_bins, tau, self.first_row)

    def want_grouped(self, w=None, b=None, allow=None, y=None, groups=None):
        sb, ok = self.sb_ok(w, b, allow, y)
        return self.pkg.collapse_topk(sb, ok, self.labels if groups is None else groups, self.k, self.min_score, self.first_row)

    def thresholds(self, w=None, b=None):
        """name -> threshold: the 100th best boosted score (exactly one row's s'), the median, -inf, NaN, above the maximum."""
        sb, ok = self.sb_ok(w, b)
        s = np.sort(sb[ok])[::-1]
        return {"100th": float(s[99]), "median": float(s[s.size // 2]), "-inf": NINF, "nan": float("nan"),
                "above": float(np.nextafter(s[0], np.float32(np.inf)))}


CONFIGS = {
    "tile_plus_one": dict(shape=(257, 512, 8), k=16, kw={}),                         # one tile of 256 rows plus one row
    "tail": dict(shape=(2003, 512, 20), k=16, kw={}),                                # rows % 4 == 3: the scalar tail
    "first_row": dict(shape=(20011, 1024, 20), k=100, kw=dict(first_row=5000)),
    "c8": dict(shape=(20011, 1024, 20), k=100, kw=dict(nnz_per_lane=8)),
    "f16": dict(shape=(2003, 512, 20), k=16, kw=dict(precision="F16")),              # without a mask: the expectation from eng.scores()
    "fixed20": dict(shape=(2003, 512, 20), k=16, kw=dict(precision="FIXED", fixed_width=20)),
}


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request, pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, CONFIGS[request.param])
    yield s
    s.eng.close()


@pytest.fixture(scope="module")
def tail(pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, CONFIGS["tail"])
    yield s
    s.eng.close()


# ---- the three calls into guarded buffers ----------------------------------------------------------------------------------------
class RangeOut(GuardedOut):
    COLUMNS = (("dev_idx", "k", "int32"), ("dev_val", "k", "float32"), ("dev_counts", 1, "int32"))  # (k: the call's capacity)


class GroupOut(GuardedOut):
    COLUMNS = (("dev_idx", "k", "int32"), ("dev_val", "k", "float32"), ("dev_grp", "k", "int32"), ("dev_n", 1, "int32"))


def _facet_out(torch, count, n_bins, best=True):
    cols = (("dev_counts", n_bins, "int32"), ("dev_totals", 1, "int32")) + ((("dev_best", 2 * n_bins, "int32"),) if best else ())
    return type("FacetOut", (GuardedOut,), {"COLUMNS": cols})(torch, count, 0)


def _finish(eng, stream):
    if stream:
        stream.synchronize()
    else:
        eng.synchronize()


def _boost_kw(w, b, stride, mask, mask_stride, stream):
    return dict(dev_weight=_p(w), dev_bias=_p(b), boost_stride=stride, dev_mask=_p(mask), mask_stride=mask_stride,
                stream=stream.cuda_stream if stream else 0)


def _range(eng, torch, dxs, taus, w=None, b=None, stride=0, capacity=None, mask=None, mask_stride=0, stream=0, plain=False, rows=0):
    """enqueue_boosted_range (plain: enqueue_range) of len(taus) queries; waits; [(count, idx[written], val[written])] per query."""
    n = len(taus)
    capacity = rows if capacity is None else capacity
    out = RangeOut(torch, n, capacity)
    dt = _dev(torch, _f32(taus))
    ptrs = out.ptrs()
    if capacity == 0:
        ptrs["dev_idx"] = ptrs["dev_val"] = 0
    torch.cuda.synchronize()
    if plain:
        eng.enqueue_range(_p(dxs), n, dt.data_ptr(), capacity=capacity, dev_mask=_p(mask), mask_stride=mask_stride,
                          stream=stream.cuda_stream if stream else 0, **ptrs)
    else:
        eng.enqueue_boosted_range(_p(dxs), n, dt.data_ptr(), capacity=capacity, **_boost_kw(w, b, stride, mask, mask_stride, stream), **ptrs)
    _finish(eng, stream)
    res = out.read()
    got = []
    for q in range(n):
        cnt = int(res["dev_counts"].view(np.uint32)[q, 0])
        kept = min(cnt, capacity)
        idx, val = res["dev_idx"].view(np.uint32)[q], res["dev_val"][q]
        assert np.all(idx[kept:] == np.uint32(0xFFFFFFF9)) and np.all(val[kept:] == -7), "something was written beyond min(count, capacity)"
        got.append((cnt, idx[:kept].copy(), val[:kept].copy()))
    return got


def _pairs(idx, val):
    return set(zip(idx.tolist(), bits(val).tolist()))


def _same_range(got, want, what=""):
    cnt, idx, val = got
    wi, wv, wn = want
    assert cnt == wn, (what, cnt, wn)
    assert idx.size == wn and len(_pairs(idx, val)) == wn, (what, "matches are not distinct")
    assert _pairs(idx, val) == _pairs(wi, wv), (what, "the set of (row, score bits) differs")


def _facets(eng, torch, dxs, taus, w=None, b=None, stride=0, n_bins=7, labels=None, best=True, mask=None, mask_stride=0, stream=0, plain=False):
    """enqueue_boosted_facets (plain: enqueue_facets); labels: a device tensor, or None for the installed ones (n_bins is then theirs);
    waits; [(counts, best_idx, best_val, total)] per query (best_*: None without dev_best)."""
    n = len(taus)
    out = _facet_out(torch, n, n_bins, best)
    dt = _dev(torch, _f32(taus))
    kw = dict(n_bins=n_bins if labels is not None else 0, dev_labels=_p(labels), **out.ptrs())
    torch.cuda.synchronize()
    if plain:
        eng.enqueue_facets(_p(dxs), n, dt.data_ptr(), dev_mask=_p(mask), mask_stride=mask_stride, stream=stream.cuda_stream if stream else 0, **kw)
    else:
        eng.enqueue_boosted_facets(_p(dxs), n, dt.data_ptr(), **_boost_kw(w, b, stride, mask, mask_stride, stream), **kw)
    _finish(eng, stream)
    res = out.read()
    got = []
    for q in range(n):
        rec = res["dev_best"].view(np.uint32)[q].reshape(n_bins, 2) if best else None
        got.append((res["dev_counts"].view(np.uint32)[q], rec[:, 0].copy() if best else None, rec[:, 1].copy().view(np.float32) if best else None,
                    int(res["dev_totals"].view(np.uint32)[q, 0])))
    return got


def _same_facets(got, want, what=""):
    assert got[3] == want[3], (what, "total", got[3], want[3])
    assert np.array_equal(got[0], want[0]), (what, "counts")
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "best rows")
        assert np.array_equal(bits(got[2]), bits(want[2])), (what, "best score bits")


def _grouped(eng, torch, dxs, count, w=None, b=None, stride=0, mask=None, mask_stride=0, stream=0, plain=False):
    """enqueue_boosted_grouped (plain: enqueue_grouped); waits; [(idx, val, grp, n)] per query."""
    out = GroupOut(torch, count, eng.k)
    torch.cuda.synchronize()
    if plain:
        eng.enqueue_grouped(_p(dxs), count, dev_mask=_p(mask), mask_stride=mask_stride, stream=stream.cuda_stream if stream else 0, **out.ptrs())
    else:
        eng.enqueue_boosted_grouped(_p(dxs), count, **_boost_kw(w, b, stride, mask, mask_stride, stream), **out.ptrs())
    _finish(eng, stream)
    res = out.read()
    return [(res["dev_idx"].view(np.uint32)[q], res["dev_val"][q], res["dev_grp"].view(np.uint32)[q], int(res["dev_n"][q, 0])) for q in range(count)]


def _same_grouped(got, want, what=""):
    assert got[3] == want[3], (what, "n", got[3], want[3])
    assert np.array_equal(got[0], want[0]), (what, "rows")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "score bits")
    assert np.array_equal(got[2], want[2]), (what, "group ids")


# ---- random boosts, thresholds, identities: every configuration ------------------------------------------------------------------------
def test_random_weight_bias_and_thresholds(pkg, setup):
    import torch
    s, eng = setup, setup.eng
    w, b = s.random_boost(1)
    dw, db = _dev(torch, w), _dev(torch, b)
    assert (~s.present).sum() > 0 and s.present.sum() > 100
    for name, hw, hb, tw, tb in (("weight", w, None, dw, None), ("bias", None, b, None, db), ("both", w, b, dw, db)):
        taus = s.thresholds(hw, hb)
        xs = torch.from_numpy(np.tile(s.x, (len(taus), 1))).cuda()
        got = _range(eng, torch, xs, list(taus.values()), tw, tb, rows=s.rows)
        for (tn, tau), g in zip(taus.items(), got):
            _same_range(g, s.want_range(tau, hw, hb), (name, tn))
        assert got[0][0] == 100 and got[2][0] == int(s.sb_ok(hw, hb)[1].sum()) and got[3][0] == 0 and got[4][0] == 0
        got = _facets(eng, torch, xs, list(taus.values()), tw, tb)
        for (tn, tau), g in zip(taus.items(), got):
            _same_facets(g, s.want_facets(tau, hw, hb), (name, tn))
        _same_grouped(_grouped(eng, torch, s.dx, 1, tw, tb)[0], s.want_grouped(hw, hb), name)


def test_identities_are_the_plain_forms(pkg, setup):
    import torch
    s, eng = setup, setup.eng
    taus = [v for v in s.thresholds().values()]
    xs = torch.from_numpy(np.tile(s.x, (len(taus), 1))).cuda()
    ones, nzero = _dev(torch, np.ones(s.rows, dtype=np.float32)), _dev(torch, np.full(s.rows, -0.0, dtype=np.float32))
    served = s.fp32  # (range_kernel and facet_kernel are fp32 kernels: the other value types have no plain form to compare with)
    plain_r = _range(eng, torch, xs, taus, plain=True, rows=s.rows) if served else None
    plain_f = _facets(eng, torch, xs, taus, plain=True) if served else None
    plain_g = _grouped(eng, torch, s.dx, 1, plain=True)[0]
    for what, w, b in (("w = 1", ones, None), ("b = -0.0", None, nzero)):
        got_r, got_f = _range(eng, torch, xs, taus, w, b, rows=s.rows), _facets(eng, torch, xs, taus, w, b)
        for q, tau in enumerate(taus):
            _same_range(got_r[q], s.want_range(tau), (what, tau))
            _same_facets(got_f[q], s.want_facets(tau), (what, tau))
            if served:
                assert got_r[q][0] == plain_r[q][0] and _pairs(*got_r[q][1:]) == _pairs(*plain_r[q][1:]), (what, tau, "enqueue_range")
                _same_facets(got_f[q], plain_f[q], (what, tau, "enqueue_facets"))
        got_g = _grouped(eng, torch, s.dx, 1, w, b)[0]
        _same_grouped(got_g, plain_g, (what, "enqueue_grouped"))
        _same_grouped(got_g, s.want_grouped(), what)


def test_identities_with_random_signs(pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, dict(shape=(2003, 512, 20), k=16, kw=dict(min_score=NINF), signs=True))
    s.min_score = NINF
    assert (s.y[s.present] < 0).sum() > 100 and (s.y[s.present] > 0).sum() > 100
    taus = list(s.thresholds().values()) + [0.0, -0.05]
    xs = torch.from_numpy(np.tile(s.x, (len(taus), 1))).cuda()
    ones, nzero = _dev(torch, np.ones(s.rows, dtype=np.float32)), _dev(torch, np.full(s.rows, -0.0, dtype=np.float32))
    plain_r, plain_f = _range(s.eng, torch, xs, taus, plain=True, rows=s.rows), _facets(s.eng, torch, xs, taus, plain=True)
    plain_g = _grouped(s.eng, torch, s.dx, 1, plain=True)[0]
    for what, w, b in (("w = 1", ones, None), ("b = -0.0", None, nzero)):
        got_r, got_f = _range(s.eng, torch, xs, taus, w, b, rows=s.rows), _facets(s.eng, torch, xs, taus, w, b)
        for q, tau in enumerate(taus):
            _same_range(got_r[q], s.want_range(tau), (what, tau))
            assert got_r[q][0] == plain_r[q][0] and _pairs(*got_r[q][1:]) == _pairs(*plain_r[q][1:]), (what, tau)
            _same_facets(got_f[q], plain_f[q], (what, tau))
        _same_grouped(_grouped(s.eng, torch, s.dx, 1, w, b)[0], plain_g, what)
        _same_grouped(plain_g, s.want_grouped(), what)
    minus = np.full(s.rows, -1.0, dtype=np.float32)  # w = -1: the rows at or below a raw threshold
    _same_range(_range(s.eng, torch, s.dx, [0.05], _dev(torch, minus), rows=s.rows)[0], s.want_range(0.05, minus), "w = -1")
    s.eng.close()


# ---- the range sink ------------------------------------------------------------------------------------------------------------------
def test_capacity_smaller_than_the_count(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    w, b = s.random_boost(2)
    dw, db = _dev(torch, w), _dev(torch, b)
    tau = s.thresholds(w, b)["median"]
    want = s.want_range(tau, w, b)
    for cap in (1, 37, want[2] - 1, want[2], want[2] + 5):
        cnt, idx, val = _range(eng, torch, s.dx, [tau], dw, db, capacity=cap)[0]  # (guard zones and the words beyond: _range)
        assert cnt == want[2] and idx.size == min(cap, want[2]), (cap, cnt, idx.size)
        got = _pairs(idx, val)
        assert len(got) == idx.size and got <= _pairs(want[0], want[1]), (cap, "distinct matches of the expected set")
    assert _range(eng, torch, s.dx, [tau, NINF], dw, db, capacity=0)[0][0] == want[2]  # capacity = 0 with NULL outputs: the count alone


def test_overflow_nan_and_subnormal_rows(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    x = (s.x * np.float32(1024.0)).astype(np.float32)  # (scores large enough for 3e38 * score to overflow)
    y, dx = s.scores_of(x), torch.from_numpy(x).cuda()
    w, b = s.random_boost(3)
    top = np.argsort(np.where(s.present, pkg.boost_scores(y, w, b), -np.inf))[::-1][:8]
    w[top[:4]] = 3e38      # the product overflows
    b[top[4:8]] = np.nan   # a NaN bias, given through the device pointer
    sb, ok = s.sb_ok(w, b, y=y)
    assert np.all(sb[top] == -np.inf) and not ok[top].any()
    dw, db = _dev(torch, w), _dev(torch, b)
    groups = np.arange(s.rows, dtype=np.uint32) // 3
    dlab = _dev(torch, groups, np.uint32)
    n_bins = int(groups.max()) + 1
    for tau in (NINF, float(np.sort(sb[ok])[::-1][50])):
        got = _range(eng, torch, dx, [tau], dw, db, rows=s.rows)[0]
        _same_range(got, s.want_range(tau, w, b, y=y), ("overflow and NaN", tau))
        assert not set((top + s.first_row).tolist()) & set(got[1].tolist())
        f = _facets(eng, torch, dx, [tau], dw, db, n_bins=n_bins, labels=dlab)[0]
        _same_facets(f, s.want_facets(tau, w, b, y=y, labels=groups, n_bins=n_bins), ("overflow and NaN", tau))
        assert f[3] == got[0] and not set((top + s.first_row).tolist()) & set(f[1][f[0] > 0].tolist())
    eng.set_groups(groups)
    g = _grouped(eng, torch, dx, 1, dw, db)[0]
    _same_grouped(g, s.want_grouped(w, b, y=y, groups=groups), "overflow and NaN")
    assert not set((top + s.first_row).tolist()) & set(g[0][:g[3]].tolist())
    # ... and the grouped path's array holds no leftover of them: the same query without a boost is enqueue_grouped's
    _same_grouped(_grouped(eng, torch, s.dx, 1, plain=True)[0], s.want_grouped(groups=groups), "grouped, behind it")
    eng.set_groups(s.labels, 7)
    # subnormal boosted scores are kept: distinct values, no flush to zero
    w = np.full(s.rows, 2.0 ** -130, dtype=np.float32)
    sb, ok = s.sb_ok(w)
    vals = np.sort(sb[ok])[::-1]
    assert vals[0] < 2.0 ** -126 and vals[60] > 0 and np.unique(vals[:60]).size > 30
    tau = float(vals[40])
    got = _range(eng, torch, s.dx, [tau], _dev(torch, w), rows=s.rows)[0]
    _same_range(got, s.want_range(tau, w), "subnormal products")
    assert got[0] >= 41 and np.all(got[2] > 0)
    _same_facets(_facets(eng, torch, s.dx, [tau], _dev(torch, w))[0], s.want_facets(tau, w), "subnormal products")
    g = _grouped(eng, torch, s.dx, 1, _dev(torch, w))[0]
    _same_grouped(g, s.want_grouped(w), "subnormal products")
    assert g[3] == 7 and np.all(g[1][:7] > 0) and np.all(g[1][:7] < 2.0 ** -126)


def test_ties_go_to_the_larger_row_id(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    zero = np.zeros(s.rows, dtype=np.float32)
    three = np.random.default_rng(6).choice(np.array([0.25, 0.5, 0.75], dtype=np.float32), s.rows)
    dz, d3 = _dev(torch, zero), _dev(torch, three)
    for tau in (0.5, 0.75, 0.25, 0.8):
        _same_range(_range(eng, torch, s.dx, [tau], dz, d3, rows=s.rows)[0], s.want_range(tau, zero, three), ("three classes", tau))
        f = _facets(eng, torch, s.dx, [tau], dz, d3)[0]
        _same_facets(f, s.want_facets(tau, zero, three), ("three classes", tau))
        if tau <= 0.75:
            for lab in range(7):  # each bin's best: the largest row id among its rows of the best class
                mine = np.flatnonzero(s.present & (s.labels == lab) & (three == 0.75))
                assert f[1][lab] == mine.max() + s.first_row and f[2][lab] == 0.75
    g = _grouped(eng, torch, s.dx, 1, dz, d3)[0]
    _same_grouped(g, s.want_grouped(zero, three), "three classes")
    reps = sorted((int(np.flatnonzero(s.present & (s.labels == lab) & (three == 0.75)).max()) + s.first_row for lab in range(7)), reverse=True)
    assert g[3] == 7 and g[0][:7].tolist() == reps and np.all(g[1][:7] == 0.75)


# ---- the facet sink's regimes --------------------------------------------------------------------------------------------------------
def test_facet_regimes_labels_and_no_best(pkg, oracle):
    import torch
    for option in (None, 0):  # the default regime, and FACET_LDS_BINS=0: global atomics always
        pkg.set_option("FACET_LDS_BINS", option)
        try:
            s = _Setup(pkg, oracle, torch, CONFIGS["first_row"])
        finally:
            pkg.set_option("FACET_LDS_BINS", None)
        w, b = s.random_boost(4)
        dw, db = _dev(torch, w), _dev(torch, b)
        taus = [s.thresholds(w, b)["median"], s.thresholds(w, b)["100th"], NINF]
        xs = torch.from_numpy(np.tile(s.x, (len(taus), 1))).cuda()
        rng = np.random.default_rng(15)
        for n_bins in (7, LDS_CAP, LDS_CAP + 1):  # LDS (few bins), LDS at its capacity, one bin more: global
            labels = rng.integers(0, n_bins + n_bins // 4 + 2, s.rows).astype(np.uint32)  # (a fifth of the rows: labels >= n_bins, in the total only)
            labels[::50] = 0xFFFFFFFF
            assert (labels >= n_bins).sum() > s.rows // 10
            dlab = _dev(torch, labels, np.uint32)
            got = _facets(s.eng, torch, xs, taus, dw, db, n_bins=n_bins, labels=dlab)
            for q, tau in enumerate(taus):
                want = s.want_facets(tau, w, b, labels=labels, n_bins=n_bins)
                _same_facets(got[q], want, (option, n_bins, tau))
                assert got[q][3] > int(got[q][0].sum()) and got[q][3] == s.want_range(tau, w, b)[2]
            nb = _facets(s.eng, torch, xs, taus, dw, db, n_bins=n_bins, labels=dlab, best=False)  # dev_best = NULL
            for q in range(len(taus)):
                assert np.array_equal(nb[q][0], got[q][0]) and nb[q][3] == got[q][3], (option, n_bins, q, "without dev_best")
            off = _dev(torch, np.concatenate([[9], labels]), np.uint32)  # labels 4 bytes off a multiple of 16: the scalar loads
            torch.cuda.synchronize()
            out = _facet_out(torch, 1, n_bins)
            dt = _dev(torch, _f32(taus[:1]))
            torch.cuda.synchronize()
            s.eng.enqueue_boosted_facets(s.dx.data_ptr(), 1, dt.data_ptr(), dev_weight=dw.data_ptr(), dev_bias=db.data_ptr(), n_bins=n_bins,
                                         dev_labels=off.data_ptr() + 4, **out.ptrs())
            s.eng.synchronize()
            assert np.array_equal(out.read()["dev_counts"].view(np.uint32)[0], got[0][0]), (option, n_bins, "unaligned labels")
        got = _facets(s.eng, torch, xs, taus, dw, db)  # the labels of set_groups
        for q, tau in enumerate(taus):
            _same_facets(got[q], s.want_facets(tau, w, b), (option, "installed labels", tau))
        s.eng.close()


# ---- grouped -------------------------------------------------------------------------------------------------------------------------
def test_grouped_label_layouts(pkg, tail):
    import torch
    s, eng = tail, tail.eng
    w, b = s.random_boost(5)
    dw, db = _dev(torch, w), _dev(torch, b)
    rng = np.random.default_rng(16)
    layouts = {"contiguous": np.arange(s.rows, dtype=np.uint32) // 5, "scattered": rng.permutation(s.rows).astype(np.uint32) % 300,
               "own": np.arange(s.rows, dtype=np.uint32), "one": np.zeros(s.rows, dtype=np.uint32), "few": rng.integers(0, 5, s.rows).astype(np.uint32)}
    try:
        for name, groups in layouts.items():
            eng.set_groups(groups)
            got = _grouped(eng, torch, s.dx, 1, dw, db)[0]
            want = s.want_grouped(w, b, groups=groups)
            _same_grouped(got, want, name)
            if name == "own":  # group[r] = r: enqueue_boosted's START page
                out = support.PageOut(torch, 1, s.k)
                torch.cuda.synchronize()
                eng.enqueue_boosted(s.dx.data_ptr(), 1, dw.data_ptr(), db.data_ptr(), **out.ptrs())
                eng.synchronize()
                idx, val, n, _, _ = out.read()[0]
                assert n == got[3] == s.k and np.array_equal(idx, got[0]) and np.array_equal(bits(val), bits(got[1]))
                assert np.array_equal(got[2], got[0] - s.first_row)
            if name == "one":  # one group: the best row alone, then pads
                sb, ok = s.sb_ok(w, b)
                assert got[3] == 1 and got[0][0] == int(np.argmax(np.where(ok, sb, -np.inf))) + s.first_row
            if name in ("one", "few"):  # fewer groups than k: pads and dev_n
                n = got[3]
                assert n == (1 if name == "one" else 5) < s.k
                assert np.all(got[0][n:] == 0) and np.all(bits(got[1][n:]) == 0) and np.all(got[2][n:] == 0xFFFFFFFF)
    finally:
        eng.set_groups(s.labels, 7)


# ---- several queries, strides, masks, streams -----------------------------------------------------------------------------------------
def test_four_queries_strides_masks_and_unaligned_pointers(pkg, tail):
    import torch
    s, eng, rows = tail, tail.eng, tail.rows
    rng = np.random.default_rng(14)
    xs = np.stack([pkg.create_sample_vector(s.cols, True, False, True, 40 + i) for i in range(4)]).astype(np.float32)
    ys = [s.scores_of(xs[q]) for q in range(4)]
    stride = rows + 3  # query 1 and 3 start off a multiple of 16 bytes: the scalar loads; query 0 and 2 the 16-byte loads
    assert (stride * 4) % 16 != 0 and (2 * stride * 4) % 16 == 0
    w = np.full((4, stride), np.nan, dtype=np.float32)  # (the three floats between two queries' arrays are never read)
    b = np.full((4, stride), np.nan, dtype=np.float32)
    w[:, :rows] = rng.uniform(0.5, 2.0, (4, rows))
    b[:, :rows] = rng.uniform(-1.0, 1.0, (4, rows))
    dxs, dw, db = torch.from_numpy(xs).cuda(), _dev(torch, w.ravel()), _dev(torch, b.ravel())
    assert dw.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    allows = [rng.random(rows) < 0.5, rng.random(rows) < 0.001, np.zeros(rows, dtype=bool), None]
    allows[1][np.flatnonzero(s.present)[:2]] = True  # (0.1 %: a few rows, two of them surely present)
    mwords = (rows + 31) // 32
    mask = np.stack([pkg.row_mask(rows, a) for a in allows])
    dmask = _dev(torch, mask.ravel(), np.uint32)
    allows[3] = np.ones(rows, dtype=bool)

    def check(tag, wq, bq, allow_of, **kw):
        sbs = [s.sb_ok(wq(q), bq(q), allow_of(q), ys[q]) for q in range(4)]
        taus = [float(np.sort(sb[ok])[::-1][min(100, int(ok.sum()) - 1)]) if ok.any() else 0.0 for sb, ok in sbs]  # per-query thresholds
        got = _range(eng, torch, dxs, taus, rows=rows, **kw)
        for q in range(4):
            _same_range(got[q], s.want_range(taus[q], wq(q), bq(q), allow_of(q), ys[q]), (tag, "range", q))
        got = _facets(eng, torch, dxs, taus, **kw)
        for q in range(4):
            _same_facets(got[q], s.want_facets(taus[q], wq(q), bq(q), allow_of(q), ys[q]), (tag, "facets", q))
        got = _grouped(eng, torch, dxs, 4, **{k: v for k, v in kw.items()})
        for q in range(4):
            _same_grouped(got[q], s.want_grouped(wq(q), bq(q), allow_of(q), ys[q]), (tag, "grouped", q))

    none = lambda q: None
    check("stride rows + 3", lambda q: w[q, :rows], lambda q: b[q, :rows], none, w=dw, b=db, stride=stride)
    check("stride 0", lambda q: w[0, :rows], lambda q: b[0, :rows], none, w=dw, b=db, stride=0)
    check("a per-query bias alone", none, lambda q: b[q, :rows], none, b=db, stride=stride)
    check("per-query masks", lambda q: w[q, :rows], lambda q: b[q, :rows], lambda q: allows[q], w=dw, b=db, stride=stride, mask=dmask, mask_stride=mwords)
    check("one mask", lambda q: w[q, :rows], lambda q: b[q, :rows], lambda q: allows[0], w=dw, b=db, stride=stride, mask=dmask, mask_stride=0)
    # arrays that start 4 and 12 bytes off a multiple of 16
    off_w, off_b = _dev(torch, np.concatenate([[np.nan], w[2, :rows]])), _dev(torch, np.concatenate([[np.nan] * 3, b[2, :rows]]))
    sb, ok = s.sb_ok(w[2, :rows], b[2, :rows], y=ys[0])
    tau = float(np.sort(sb[ok])[::-1][100])

    class Off:  # (a tensor's view whose data_ptr is moved)
        def __init__(self, t, by):
            self.t, self.by = t, by

        def data_ptr(self):
            return self.t.data_ptr() + self.by

    ow, ob = Off(off_w, 4), Off(off_b, 12)
    _same_range(_range(eng, torch, dxs, [tau], ow, ob, rows=rows)[0], s.want_range(tau, w[2, :rows], b[2, :rows], y=ys[0]), "unaligned pointers")
    _same_facets(_facets(eng, torch, dxs, [tau], ow, ob)[0], s.want_facets(tau, w[2, :rows], b[2, :rows], y=ys[0]), "unaligned pointers")
    _same_grouped(_grouped(eng, torch, dxs, 1, ow, ob)[0], s.want_grouped(w[2, :rows], b[2, :rows], y=ys[0]), "unaligned pointers")


def test_installed_boost_run_forms_streams_and_repeats(pkg, tail):
    import torch
    s, eng, L = tail, tail.eng, pkg._lib
    w, b = s.random_boost(5)
    tau = s.thresholds(w, b)["100th"]
    eng.set_boost(None, None)
    dt = _dev(torch, _f32([tau]))
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert status_of(pkg, eng.enqueue_boosted_range, s.dx.data_ptr(), 1, dt.data_ptr(), cnt.data_ptr()) == L.ERR_STATE  # both NULL, none installed
    assert status_of(pkg, eng.run_boosted_range, tau) == L.ERR_STATE
    assert status_of(pkg, eng.run_boosted_facets, tau) == L.ERR_STATE
    assert status_of(pkg, eng.run_boosted_grouped) == L.ERR_STATE
    eng.set_boost(w, b)
    wr, wf, wg = s.want_range(tau, w, b), s.want_facets(tau, w, b), s.want_grouped(w, b)
    _same_range(_range(eng, torch, s.dx, [tau], rows=s.rows)[0], wr, "both NULL: the installed boost")
    _same_range(_range(eng, torch, None, [tau], rows=s.rows)[0], wr, "the installed vector and the installed boost")
    _same_facets(_facets(eng, torch, None, [tau])[0], wf, "installed vector, boost and labels")
    _same_grouped(_grouped(eng, torch, None, 1)[0], wg, "installed vector and boost")
    val, idx = eng.run_boosted_range(tau)  # sorted like run_range: the restatement's own order
    assert eng.last_range_count == wr[2] == 100 and np.array_equal(idx, wr[0]) and np.array_equal(bits(val), bits(wr[1]))
    val, idx = eng.run_boosted_range(tau, capacity=10)
    assert eng.last_range_count == 100 and idx.size == 10 and _pairs(idx, val) <= _pairs(wr[0], wr[1])
    _same_facets(eng.run_boosted_facets(tau), wf, "run_boosted_facets")
    val, idx, grp = eng.run_boosted_grouped()
    n = wg[3]
    assert idx.size == n and np.array_equal(idx, wg[0][:n]) and np.array_equal(bits(val), bits(wg[1][:n])) and np.array_equal(grp, wg[2][:n])
    allow = np.random.default_rng(2).random(s.rows) < 0.3
    val, idx = eng.run_boosted_range(tau, allow=allow, weight=w)  # the weight alone: the bias installed before is gone
    wa = s.want_range(tau, w, None, allow)
    assert np.array_equal(idx, wa[0]) and np.array_equal(bits(val), bits(wa[1]))
    _same_facets(eng.run_boosted_facets(tau, allow=allow, bias=b), s.want_facets(tau, None, b, allow), "run_boosted_facets, mask, bias alone")
    val, idx, grp = eng.run_boosted_grouped(allow=allow, weight=w, bias=b)
    wa = s.want_grouped(w, b, allow)
    assert np.array_equal(idx, wa[0][:wa[3]]) and np.array_equal(bits(val), bits(wa[1][:wa[3]])) and np.array_equal(grp, wa[2][:wa[3]])
    eng.set_filter(None)
    # a caller's stream, explicit arrays and the installed ones; the same call twice gives identical bits
    side = torch.cuda.Stream()
    dw, db = _dev(torch, w), _dev(torch, b)
    for tw, tb in ((dw, db), (None, None)):
        first = (_range(eng, torch, s.dx, [tau], tw, tb, stream=side, rows=s.rows)[0], _facets(eng, torch, s.dx, [tau], tw, tb, stream=side)[0],
                 _grouped(eng, torch, s.dx, 1, tw, tb, stream=side)[0])
        _same_range(first[0], wr, "a caller's stream")
        _same_facets(first[1], wf, "a caller's stream")
        _same_grouped(first[2], wg, "a caller's stream")
        again = (_range(eng, torch, s.dx, [tau], tw, tb, stream=side, rows=s.rows)[0], _facets(eng, torch, s.dx, [tau], tw, tb, stream=side)[0],
                 _grouped(eng, torch, s.dx, 1, tw, tb, stream=side)[0])
        assert first[0][0] == again[0][0] and _pairs(*first[0][1:]) == _pairs(*again[0][1:])
        _same_facets(again[1], first[1], "twice")
        _same_grouped(again[2], first[2], "twice")
    eng.set_boost(None, None)
    # the one-shot helpers
    val, idx = pkg.boosted_range_spmv(s.m, s.x, tau, weight=w, bias=b, k=s.k)
    assert np.array_equal(idx, wr[0]) and np.array_equal(bits(val), bits(wr[1]))
    _same_facets(pkg.boosted_facet_spmv(s.m, s.x, tau, s.labels, 7, weight=w, bias=b, k=s.k), wf, "boosted_facet_spmv")
    val, idx, grp = pkg.boosted_grouped_spmv(s.m, s.x, s.labels, k=s.k, weight=w, bias=b)
    assert np.array_equal(idx, wg[0][:wg[3]]) and np.array_equal(bits(val), bits(wg[1][:wg[3]])) and np.array_equal(grp, wg[2][:wg[3]])
    # cosine: set_cosine() then the radius query, against the restatement on the device's own weights
    eng.set_cosine()
    cw = eng.row_stats(L.ROW_INV_L2)
    ct = float(np.sort(s.sb_ok(cw)[0][s.present])[::-1][49])
    val, idx = eng.run_boosted_range(ct)
    wc = s.want_range(ct, cw)
    assert wc[2] >= 50 and np.array_equal(idx, wc[0]) and np.array_equal(bits(val), bits(wc[1]))
    cv, ci = pkg.cosine_range_spmv(s.m, s.x * 3.0, ct, k=s.k)
    assert ci.size >= 45 and set(ci.tolist()) <= set(s.want_range(float(np.nextafter(np.float32(ct), np.float32(-1))) - 1e-6, cw)[0].tolist())
    eng.set_boost(None, None)


def test_engine_state_untouched(pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, dict(shape=(20011, 1024, 20), k=100, kw={}))
    eng, k, nq = s.eng, s.k, 8
    xs = np.stack([pkg.create_sample_vector(s.cols, True, False, True, 300 + i) for i in range(nq)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    w, b = s.random_boost(7)
    dw, db = _dev(torch, w), _dev(torch, b)
    ys = [s.scores_of(xs[q]) for q in range(3)]
    taus = [float(np.sort(s.sb_ok(w, b, y=ys[q])[0][s.present])[::-1][99]) for q in range(3)]

    def batch():
        bi = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        bv = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.enqueue_batch(dxs.data_ptr(), nq, bi.data_ptr(), bv.data_ptr())
        eng.synchronize()
        return bi.cpu().numpy(), bv.cpu().numpy().view(np.uint32)

    first = batch()
    before = eng.debug_counters()
    for q, g in enumerate(_range(eng, torch, dxs, taus, dw, db, rows=s.rows)):
        _same_range(g, s.want_range(taus[q], w, b, y=ys[q]), f"range {q}")
    for q, g in enumerate(_facets(eng, torch, dxs, taus, dw, db)):
        _same_facets(g, s.want_facets(taus[q], w, b, y=ys[q]), f"facets {q}")
    for q, g in enumerate(_grouped(eng, torch, dxs, 3, dw, db)):
        _same_grouped(g, s.want_grouped(w, b, y=ys[q]), f"grouped {q}")
    after = eng.debug_counters()
    assert after == before, (before, after)  # no batch or single launch, no check failed, nothing suspended
    again = batch()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    s.eng.close()


def test_errors_in_the_stated_order(pkg):
    import torch
    L = pkg._lib
    m = pkg.generate_matrix(2003, 512, 20, "gamma", 4)
    x = pkg.create_sample_vector(512, True, False, True, 2)
    rows, k = m.rows, 16
    dmask = torch.from_numpy(pkg.row_mask(rows).view(np.int32)).cuda()
    dw = _dev(torch, np.ones(rows, dtype=np.float32))
    dlab = torch.zeros(rows, dtype=torch.int32, device="cuda")
    buf = torch.zeros(4 * k, dtype=torch.int32, device="cuda")
    dt = _dev(torch, _f32([0.5, 0.5]))
    torch.cuda.synchronize()
    W, T, B, M, LAB = dw.data_ptr(), dt.data_ptr(), buf.data_ptr(), dmask.data_ptr(), dlab.data_ptr()

    def forms(eng):
        """name -> call(dev_xs, count, **kw) with valid outputs; range and facets count only."""
        return {"range": lambda xs, n, **kw: eng.enqueue_boosted_range(xs, n, kw.pop("tau", T), kw.pop("counts", B), **kw),
                "facets": lambda xs, n, **kw: eng.enqueue_boosted_facets(xs, n, kw.pop("tau", T), kw.pop("counts", B), **kw),
                "grouped": lambda xs, n, **kw: eng.enqueue_boosted_grouped(xs, n, **kw)}

    eng = pkg.SpMV(m.row, m.col, m.val, rows, 512, k=k, device=0)
    for name, call in forms(eng).items():
        assert status_of(pkg, call, 0, 1, dev_weight=W) == L.ERR_STATE      # no query vector installed (nor labels)
        assert status_of(pkg, call, 0, 1) == L.ERR_STATE                    # ... and no boost either
        assert status_of(pkg, call, 0, 2, dev_weight=W) == L.ERR_INVALID    # NULL dev_xs takes the installed vector: count must be 1
        assert status_of(pkg, call, 0, 2) == L.ERR_INVALID                  # INVALID comes before STATE
    eng.reset(x)
    for name, call in forms(eng).items():
        assert status_of(pkg, call, 0, 1) == L.ERR_STATE                    # a vector, but no boost installed
        if name != "range":
            assert status_of(pkg, call, 0, 1, dev_weight=W) == L.ERR_STATE  # a vector and a boost, but no labels
        assert status_of(pkg, call, 0, 0, dev_weight=W) == L.ERR_INVALID
        assert status_of(pkg, call, 0, -3, dev_weight=W) == L.ERR_INVALID
        assert status_of(pkg, call, 0, 1, dev_weight=W, boost_stride=-1) == L.ERR_INVALID               # a negative boost stride
        assert status_of(pkg, call, 0, 1, dev_weight=W, dev_mask=M, mask_stride=-1) == L.ERR_INVALID    # a negative mask stride
        if name != "grouped":
            assert status_of(pkg, call, 0, 1, dev_weight=W, tau=0) == L.ERR_INVALID                     # no thresholds
            assert status_of(pkg, call, 0, 1, dev_weight=W, counts=0) == L.ERR_INVALID                  # no counts
    f = forms(eng)
    for given in (dict(dev_idx=B), dict(dev_val=B), dict(dev_idx=B, dev_val=B), dict(capacity=4)):     # the range outputs partly given
        assert status_of(pkg, f["range"], 0, 1, dev_weight=W, **given) == L.ERR_INVALID
    assert status_of(pkg, f["facets"], 0, 1, dev_weight=W, dev_labels=LAB) == L.ERR_INVALID            # labels without n_bins
    assert status_of(pkg, f["facets"], 0, 1, dev_weight=W, n_bins=3) == L.ERR_INVALID                  # n_bins without labels
    assert status_of(pkg, f["facets"], 0, 1, dev_weight=W, dev_labels=LAB, n_bins=3, dev_best=B + 4) == L.ERR_INVALID  # dev_best off 8 bytes
    for given in (dict(dev_idx=B), dict(dev_idx=B, dev_val=B), dict(dev_grp=B)):                        # the grouped outputs partly given
        assert status_of(pkg, f["grouped"], 0, 1, dev_weight=W, **given) == L.ERR_INVALID
    cnt, n = C.c_uint64(5), C.c_int32(5)
    assert L.lib().tkspmv_run_boosted_range(eng._h, 0.5, 1, None, None, 0, C.byref(cnt)) == L.ERR_INVALID  # use_filter, none installed
    assert L.lib().tkspmv_run_boosted_range(eng._h, 0.5, 0, None, None, 0, None) == L.ERR_INVALID           # no count
    assert L.lib().tkspmv_run_boosted_facets(eng._h, 0.5, 1, None, None, C.byref(cnt)) == L.ERR_INVALID
    assert L.lib().tkspmv_run_boosted_grouped(eng._h, 1, None, None, None, C.byref(n)) == L.ERR_INVALID
    assert cnt.value == 5 and n.value == 5
    val, idx = eng.run_boosted_range(0.0, weight=np.ones(rows, dtype=np.float32))  # ... and the engine still answers
    assert idx.size == eng.last_range_count > 0
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 512, k=k, device=0, partitions=4, k_per_partition=8)  # the approximate per-partition path
    for name, call in forms(eng).items():
        assert status_of(pkg, call, 0, 0, dev_weight=W) == L.ERR_INVALID      # INVALID comes first ...
        assert status_of(pkg, call, 0, 1) == L.ERR_UNSUPPORTED                # ... UNSUPPORTED before STATE (no vector, no boost, no labels)
        assert status_of(pkg, call, 0, 1, dev_weight=W) == L.ERR_UNSUPPORTED
    assert status_of(pkg, eng.run_boosted_range, 0.5) == L.ERR_UNSUPPORTED
    assert status_of(pkg, eng.run_boosted_facets, 0.5) == L.ERR_UNSUPPORTED
    assert status_of(pkg, eng.run_boosted_grouped) == L.ERR_UNSUPPORTED
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 512, k=k, device=0, precision=pkg.F16)
    eng.reset(x)
    eng.run_boosted_range(0.5, weight=np.ones(rows, dtype=np.float32))  # served without a mask ...
    eng.set_boost(None, None)
    for name, call in forms(eng).items():  # ... a mask needs the filter kernels (before STATE: no boost, no labels)
        assert status_of(pkg, call, 0, 1, dev_mask=M) == L.ERR_UNSUPPORTED
        assert status_of(pkg, call, 0, 1, dev_weight=W, dev_mask=M) == L.ERR_UNSUPPORTED
    eng.close()
