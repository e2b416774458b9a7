"""Facet counts (tkspmv_enqueue_facets / tkspmv_run_facets) on the MI355X.

The expectation is facet_counts -- the contract restated in numpy, itself checked against a plain loop in test_facets_host.py --
applied to yp, present from the order-matched oracle (oracle.packed_scores of the engine's own layout, as test_gpu_range.py builds
them): counts, totals and each bin's best (row, score bits) must be EQUAL, not close. Every case runs on an engine with the default
deposit regime (the workgroup's histogram in LDS up to the column tier's capacity) and on one created under FACET_LDS_BINS=0
(global atomics always); a third, created under FACET_LDS_BINS=64, puts 64 and 65 bins on either side of the switch.
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

import support
from support import Scores, bits

pytestmark = pytest.mark.gpu

NO_FACET = 0xFFFFFFFF
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
BINS = (1, 7, 64, 1000, 200_000)


def _labels(kind, rows, n_bins, seed=0):
    rng = np.random.default_rng(1000 + seed + n_bins)
    if kind == "mod":
        return (np.arange(rows, dtype=np.int64) % n_bins).astype(np.uint32)
    lab = rng.integers(0, n_bins, rows).astype(np.uint32)
    if kind == "skewed":  # 90 % of the rows in bin 0
        lab[rng.random(rows) < 0.9] = 0
    if kind == "no_facet":  # 5 % of the rows in no bin, and a few just beyond the bins
        lab[rng.random(rows) < 0.05] = NO_FACET
        lab[rng.random(rows) < 0.01] = n_bins
    return lab


def _engines(pkg, m, k, **kw):
    """{regime: engine}: the default regime, global atomics always, and the switch at 64 bins."""
    out = {}
    for name, v in (("default", None), ("lds0", 0), ("lds64", 64)):
        pkg.set_option("FACET_LDS_BINS", v)
        try:
            out[name] = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, **kw)
        finally:
            pkg.set_option("FACET_LDS_BINS", None)
    return out


def _buffers(torch, nq, n_bins, best=True, totals=True):
    """Pattern-filled output buffers of one call, each with a guard element on either side."""
    n = nq * n_bins
    dc = torch.from_numpy(np.full(n + 2, FILL32, dtype=np.uint32).view(np.int32)).cuda()
    db = torch.from_numpy(np.full(n + 2, FILL64, dtype=np.uint64).view(np.int64)).cuda() if best else None
    dt = torch.from_numpy(np.full(nq + 2, FILL32, dtype=np.uint32).view(np.int32)).cuda() if totals else None
    return dc, db, dt


def _facets(torch, eng, dxs, nq, dthr, dlab, n_bins, best=True, totals=True, dmask=None, stride=0, stream=None, bufs=None):
    """One enqueue_facets call into _buffers. Returns (counts[nq, n_bins], best[nq, n_bins, 2] or None, totals[nq] or None) after
    checking that the guards still hold the pattern. bufs given (filled and waited for by the caller): nothing is waited for, neither
    in front of the call nor behind it, and the function that reads the buffers is returned instead."""
    sync = bufs is None
    if bufs is None:
        bufs = _buffers(torch, nq, n_bins, best, totals)
        torch.cuda.synchronize()
    dc, db, dt = bufs
    eng.enqueue_facets(dxs, nq, dthr.data_ptr(), dc.data_ptr() + 4, n_bins, dlab.data_ptr() if dlab is not None else 0,
                       db.data_ptr() + 8 if best else 0, dt.data_ptr() + 4 if totals else 0,
                       dmask.data_ptr() if dmask is not None else 0, stride, stream.cuda_stream if stream is not None else 0)

    def read():
        hc = dc.cpu().numpy().view(np.uint32)
        assert hc[0] == FILL32 and hc[-1] == FILL32, "dev_counts was written outside count * n_bins entries"
        hb = ht = None
        if best:
            hb = db.cpu().numpy().view(np.uint64)
            assert hb[0] == FILL64 and hb[-1] == FILL64, "dev_best was written outside count * n_bins entries"
            hb = hb[1:-1].copy().view(np.uint32).reshape(nq, n_bins, 2)
        if totals:
            ht = dt.cpu().numpy().view(np.uint32)
            assert ht[0] == FILL32 and ht[-1] == FILL32, "dev_totals was written outside count entries"
            ht = ht[1:-1].copy()
        return hc[1:-1].copy().reshape(nq, n_bins), hb, ht
    if not sync:
        return read
    if stream is not None:
        stream.synchronize()
    else:
        eng.synchronize()
    return read()


def _expect(pkg, scores, labels, n_bins, tv, first_row=0, allows=None):
    """facet_counts per query: scores = [(yp, present)] (one pair: the same for every query), allows likewise."""
    cs, bs, ts = [], [], []
    for i, t in enumerate(tv):
        yp, present = scores[i if len(scores) > 1 else 0]
        allow = None if allows is None else allows[i if len(allows) > 1 else 0]
        c, bi, bv, tot = pkg.facet_counts(yp, present, labels, n_bins, t, first_row=first_row, allow=allow)
        cs.append(c)
        bs.append(np.stack([bi, bits(bv)], axis=1))
        ts.append(tot)
    return np.stack(cs), np.stack(bs), np.array(ts, dtype=np.uint32)


def _same(got, exp, label):
    (gc, gb, gt), (ec, eb, et) = got, exp
    assert np.array_equal(gc, ec), f"{label}: counts differ in {np.count_nonzero(gc != ec)} bins"
    if gt is not None:
        assert np.array_equal(gt, et), f"{label}: totals {gt.tolist()} != {et.tolist()}"
    if gb is not None:
        bad = np.argwhere((gb != eb).any(axis=2))
        assert bad.size == 0, f"{label}: best differs in {len(bad)} bins, first {bad[0].tolist()}: {gb[tuple(bad[0])].tolist()} != {eb[tuple(bad[0])].tolist()}"


SHAPES = [
    (1000, 512, {}),
    (100_000, 1024, {}),
    (20_000, 4096, {}),
    (30_000, 16384, {}),
    (50_000, 1024, {"nnz_per_lane": 8}),
    (50_000, 1024, {"first_row": 5000}),
]
IDS = ["1000x512", "100kx1024", "20kx4096", "30kx16384", "c8", "first_row"]


class _Case:
    """A shape's matrix, its three engines, one query vector with the oracle's scores and the thresholds of the issue."""
    def __init__(self, pkg, oracle, torch, rows, cols, kw):
        self.rows, self.cols, self.first_row = rows, cols, kw.get("first_row", 0)
        self.m = pkg.generate_matrix(rows, cols, 20, "gamma", rows % 97 + 3)
        self.x = np.ascontiguousarray(pkg.create_sample_vector(cols, True, False, True, 17), dtype=np.float32)
        self.engines = _engines(pkg, self.m, 100, **kw)
        eng = self.engines["default"]
        self.yp, self.present = Scores(pkg, eng, self.m)(oracle, self.x)
        s = np.sort(self.yp[self.present])[::-1]
        ranks = [r for r in (1, 100, 1000) if r <= s.size]
        self.tv = np.array([-np.inf, 0.0] + [s[r - 1] for r in ranks] + [np.nextafter(np.float32(s[0]), np.float32(np.inf)), np.nan], dtype=np.float32)
        self.nq = len(self.tv)
        self.dthr = torch.from_numpy(self.tv).cuda()
        self.dxs = torch.from_numpy(np.tile(self.x, (self.nq, 1))).cuda()
        eng.reset(self.x)
        eng()
        _, self.topk = eng.read_result()

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    import torch
    made = {}

    def get(i):
        if i not in made:
            rows, cols, kw = SHAPES[i]
            made[i] = _Case(pkg, oracle, torch, rows, cols, kw)
        return made[i]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=IDS)
def test_facets_match_model(pkg, cases, shape):
    """Every kind of labels at every number of bins, at -inf, 0.0, the 1st / 100th / 1000th best score, above the maximum and NaN in one
    call, in both regimes; 64 and 65 bins on the engine that switches at 64."""
    import torch
    c = cases(shape)
    for kind in ("mod", "uniform", "skewed", "no_facet"):
        for n_bins in BINS + (65,):
            if n_bins == 65 and kind != "uniform":
                continue
            lab = _labels(kind, c.rows, n_bins)
            dlab = torch.from_numpy(lab.view(np.int32)).cuda()
            exp = _expect(pkg, [(c.yp, c.present)], lab, n_bins, c.tv, c.first_row)
            assert exp[2][0] == int(c.present.sum()) and exp[2][-1] == 0 and exp[2][-2] == 0  # -inf: every row with entries; above the maximum, NaN: none
            regimes = ("default", "lds0", "lds64") if n_bins in (64, 65) else ("default", "lds0")
            for r in regimes:
                got = _facets(torch, c.engines[r], c.dxs.data_ptr(), c.nq, c.dthr, dlab, n_bins)
                _same(got, exp, f"{IDS[shape]}/{kind}/{n_bins}/{r}")


@pytest.mark.parametrize("shape,cap", [(1, 4096), (2, 4096), (3, 512)], ids=["1024:4096", "4096:4096", "16384:512"])
def test_capacity_edge(pkg, cases, shape, cap):
    """n_bins at the column tier's built-in capacity (the whole histogram in use, the last bin included) and one above it (the first
    number of bins that goes with global atomics on a default engine), against the model and the engine of global atomics always."""
    import torch
    c = cases(shape)
    for n_bins in (cap, cap + 1):
        lab = _labels("uniform", c.rows, n_bins, seed=8)
        lab[:: 97] = n_bins - 1  # (the last bin is never empty)
        dlab = torch.from_numpy(lab.view(np.int32)).cuda()
        exp = _expect(pkg, [(c.yp, c.present)], lab, n_bins, c.tv, c.first_row)
        assert exp[0][0][n_bins - 1] > 0
        for r in ("default", "lds0"):
            _same(_facets(torch, c.engines[r], c.dxs.data_ptr(), c.nq, c.dthr, dlab, n_bins), exp, f"{IDS[shape]}/edge/{n_bins}/{r}")


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=IDS)
def test_masks(pkg, cases, shape):
    """The four masks of test_gpu_filter.py, one for every query (stride 0) and one per query (stride)."""
    import torch
    c = cases(shape)
    masks = support.masks(c.rows, c.topk, c.first_row, c.rows)
    for n_bins in (7, 1000):
        lab = _labels("no_facet", c.rows, n_bins, seed=5)
        dlab = torch.from_numpy(lab.view(np.int32)).cuda()
        for name, allow in masks.items():
            dmask = torch.from_numpy(pkg.row_mask(c.rows, allow).view(np.int32)).cuda()
            exp = _expect(pkg, [(c.yp, c.present)], lab, n_bins, c.tv, c.first_row, [allow])
            for r in ("default", "lds0"):
                _same(_facets(torch, c.engines[r], c.dxs.data_ptr(), c.nq, c.dthr, dlab, n_bins, dmask=dmask), exp, f"{IDS[shape]}/{name}/{n_bins}/{r}")
        per_q = [list(masks.values())[i % 4] for i in range(c.nq)]
        words = np.stack([pkg.row_mask(c.rows, a) for a in per_q])
        dmask = torch.from_numpy(words.view(np.int32)).cuda()
        exp = _expect(pkg, [(c.yp, c.present)], lab, n_bins, c.tv, c.first_row, per_q)
        for r in ("default", "lds0"):
            _same(_facets(torch, c.engines[r], c.dxs.data_ptr(), c.nq, c.dthr, dlab, n_bins, dmask=dmask, stride=words.shape[1]), exp,
                  f"{IDS[shape]}/per_query/{n_bins}/{r}")


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=IDS)
def test_agrees_with_range(pkg, cases, shape):
    """The engine against itself: the rows enqueue_range returns, counted by label, are dev_counts; its count is dev_totals."""
    import torch
    c = cases(shape)
    eng = c.engines["default"]
    n_bins = 64
    lab = _labels("no_facet", c.rows, n_bins, seed=9)
    dlab = torch.from_numpy(lab.view(np.int32)).cuda()
    tv = c.tv[[1, 3]] if c.nq > 3 else c.tv[[1, 2]]  # 0.0 and the 100th best score
    dthr = torch.from_numpy(np.ascontiguousarray(tv)).cuda()
    cap = c.rows
    dcnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    didx = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
    dval = torch.zeros((2, cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_range(c.dxs.data_ptr(), 2, dthr.data_ptr(), dcnt.data_ptr(), didx.data_ptr(), dval.data_ptr(), cap)
    eng.synchronize()
    rc = dcnt.cpu().numpy().view(np.uint32)
    ri = didx.cpu().numpy().view(np.uint32)
    for r in ("default", "lds0"):
        gc, gb, gt = _facets(torch, c.engines[r], c.dxs.data_ptr(), 2, dthr, dlab, n_bins)
        for i in range(2):
            hit = lab[ri[i, :rc[i]].astype(np.int64) - c.first_row]
            assert np.array_equal(np.bincount(hit[hit < n_bins], minlength=n_bins), gc[i]), (IDS[shape], r, i)
            assert rc[i] == gt[i] and rc[i] > 0


@pytest.fixture(scope="module")
def seq(pkg, oracle):
    """50 000 x 1024 with four stream copies, 70 query vectors and their scores; the engines of both regimes."""
    rows, cols, nq = 50_000, 1024, 70
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 12)
    engines = _engines(pkg, m, 100, stream_replicas=4)
    engines.pop("lds64").close()
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 300 + i) for i in range(nq)]).astype(np.float32)
    sc = Scores(pkg, engines["default"], m)
    scores = [sc(oracle, xs[i]) for i in range(nq)]
    yield m, engines, xs, scores
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("nq", [33, 70])
def test_sequences(pkg, seq, nq):
    """More queries than one launch takes, per-query thresholds; a query at -inf directly followed by one above the maximum, whose bins
    must all be 0 (the histogram is cleared between the queries of a launch); the same call again gives the same arrays."""
    import torch
    m, engines, xs, scores = seq
    ranks = [10, 100, 1000, 3, 20_000]
    tv = np.array([np.sort(scores[i][0][scores[i][1]])[::-1][ranks[i % len(ranks)] - 1] for i in range(nq)], dtype=np.float32)
    for j in (4, 30, nq - 2):  # inside a launch, across the 32-query boundary (30, 31 | 32), at the end
        tv[j] = -np.inf
        tv[j + 1] = np.nextafter(np.float32(scores[j + 1][0][scores[j + 1][1]].max()), np.float32(np.inf))
    tv[31], tv[32] = -np.inf, np.nextafter(np.float32(scores[32][0][scores[32][1]].max()), np.float32(np.inf))
    dxs = torch.from_numpy(xs[:nq]).cuda()
    dthr = torch.from_numpy(tv).cuda()
    for n_bins in (7, 1000, 200_000):
        lab = _labels("skewed", m.rows, n_bins, seed=2)
        dlab = torch.from_numpy(lab.view(np.int32)).cuda()
        exp = _expect(pkg, scores[:nq], lab, n_bins, tv)
        for j in (5, 31 + 1, nq - 1):
            assert not exp[0][j].any() and exp[0][j - 1].sum() == scores[j - 1][1].sum()
        for r, eng in engines.items():
            got = _facets(torch, eng, dxs.data_ptr(), nq, dthr, dlab, n_bins)
            _same(got, exp, f"seq{nq}/{n_bins}/{r}")
            again = _facets(torch, eng, dxs.data_ptr(), nq, dthr, dlab, n_bins)
            assert all(np.array_equal(a, b) for a, b in zip(got, again)), f"seq{nq}/{n_bins}/{r}: a rerun differs"


def test_optional_outputs_and_extent(pkg, cases):
    """dev_best = NULL and dev_totals = NULL each work, alone and together; _facets checks the guards around every buffer."""
    import torch
    c = cases(1)
    for n_bins in (7, 200_000):
        lab = _labels("uniform", c.rows, n_bins, seed=3)
        dlab = torch.from_numpy(lab.view(np.int32)).cuda()
        exp = _expect(pkg, [(c.yp, c.present)], lab, n_bins, c.tv, c.first_row)
        for r in ("default", "lds0"):
            for best, totals in ((False, True), (True, False), (False, False)):
                got = _facets(torch, c.engines[r], c.dxs.data_ptr(), c.nq, c.dthr, dlab, n_bins, best=best, totals=totals)
                assert (got[1] is None) == (not best) and (got[2] is None) == (not totals)
                _same(got, exp, f"optional/{n_bins}/{r}/{best}/{totals}")


def _batch(torch, eng, dxs, nq, then=None):
    out_i = torch.zeros((nq, eng.k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((nq, eng.k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    reads = then() if then is not None else []  # (not waited for: right behind the batch launch)
    eng.synchronize()
    torch.cuda.synchronize()
    return out_i.cpu().numpy().view(np.uint32).copy(), out_v.cpu().numpy().copy(), reads


def test_no_cross_talk(pkg, oracle):
    """A facet call left unwaited right behind enqueue_batch, on the engine's stream and on a caller's stream: the batch results equal
    a run without it (and the oracle), a later tkspmv_run too, and the facet calls' own output is correct."""
    import torch
    rows, cols, k, nq = 100_000, 1024, 100, 8
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 77)
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 500 + i) for i in range(nq)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    n_bins = 16
    lab = _labels("uniform", rows, n_bins, seed=4)
    dlab = torch.from_numpy(lab.view(np.int32)).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    sc = Scores(pkg, eng, m)
    scores = [sc(oracle, xs[i]) for i in range(nq)]
    tv = np.array([np.sort(scores[q][0][scores[q][1]])[::-1][499] for q in range(nq)], dtype=np.float32)
    dthr = torch.from_numpy(tv).cuda()
    side = torch.cuda.Stream()

    def facets_behind():
        return [_facets(torch, eng, dxs.data_ptr(), nq, dthr, dlab, n_bins, bufs=bufs[0]),
                _facets(torch, eng, dxs.data_ptr(), nq, dthr, dlab, n_bins, stream=side, bufs=bufs[1])]
    bufs = [_buffers(torch, nq, n_bins) for _ in range(2)]  # (_batch waits for torch before it enqueues)
    bi, bv, reads = _batch(torch, eng, dxs, nq, facets_behind)
    side.synchronize()
    eng.reset(xs[3])
    eng()
    rv, ri = eng.read_result()
    eng.close()
    ref = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    ei, ev, _ = _batch(torch, ref, dxs, nq)
    ref.reset(xs[3])
    ref()
    fv, fi = ref.read_result()
    ref.close()
    assert np.array_equal(bi, ei) and np.array_equal(bits(bv), bits(ev))
    assert np.array_equal(ri, fi) and np.array_equal(bits(rv), bits(fv))
    for q in range(nq):
        oi, ov = oracle.select_topk(*scores[q], k)
        assert np.array_equal(bi[q], oi) and np.array_equal(bits(bv[q]), bits(ov))
    exp = _expect(pkg, scores, lab, n_bins, tv)
    for name, read in zip(("engine_stream", "callers_stream"), reads):
        _same(read(), exp, f"cross_talk/{name}")


def test_installed_labels(pkg, oracle, cases):
    """set_groups + dev_labels = NULL, run_facets with and without allow, facet_spmv; a grouped query before and after is unchanged."""
    import torch
    c = cases(5)  # first_row = 5000
    eng = c.engines["default"]
    n_groups = 300
    lab = _labels("skewed", c.rows, n_groups, seed=6)
    eng.set_groups(lab, n_groups)
    gv0, gi0, gg0 = eng.run_grouped(vec=c.x)
    exp = _expect(pkg, [(c.yp, c.present)], lab, n_groups, c.tv, c.first_row)
    n = c.nq * n_groups  # (dev_labels = NULL, n_bins = 0: the outputs hold n_groups bins per query)
    dc = torch.zeros((n,), dtype=torch.int32, device="cuda")
    db = torch.zeros((n,), dtype=torch.int64, device="cuda")
    dt = torch.zeros((c.nq,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_facets(c.dxs.data_ptr(), c.nq, c.dthr.data_ptr(), dc.data_ptr(), 0, 0, db.data_ptr(), dt.data_ptr())
    eng.synchronize()
    _same((dc.cpu().numpy().view(np.uint32).reshape(c.nq, n_groups), db.cpu().numpy().view(np.uint32).reshape(c.nq, n_groups, 2),
           dt.cpu().numpy().view(np.uint32)), exp, "installed/enqueue")
    t = float(c.tv[3])
    counts, bi, bv, total = eng.run_facets(t, vec=c.x)
    assert np.array_equal(counts, exp[0][3]) and np.array_equal(bi, exp[1][3][:, 0]) and np.array_equal(bits(bv), exp[1][3][:, 1]) and total == exp[2][3]
    allow = np.random.default_rng(21).random(c.rows) < 0.3
    ec, ei, ev, et = pkg.facet_counts(c.yp, c.present, lab, n_groups, -np.inf, first_row=c.first_row, allow=allow)
    counts, bi, bv, total = eng.run_facets(-np.inf, allow=allow)
    assert np.array_equal(counts, ec) and np.array_equal(bi, ei) and np.array_equal(bits(bv), bits(ev)) and total == et
    eng.set_filter(None)
    gv1, gi1, gg1 = eng.run_grouped()
    assert np.array_equal(gi0, gi1) and np.array_equal(bits(gv0), bits(gv1)) and np.array_equal(gg0, gg1)
    eng.set_groups(None)
    # the one-shot helper
    small = pkg.generate_matrix(1000, 512, 20, "gamma", 5)
    x = pkg.create_sample_vector(512, True, False, True, 6)
    labs = (np.arange(1000) % 5).astype(np.uint32)
    counts, bi, bv, total = pkg.facet_spmv(small, x, 0.0, labs, device=0)
    y, p = oracle.scores_f64(small.row, small.col, small.val, x, small.rows)
    assert counts.tolist() == np.bincount(labs[p.astype(bool)], minlength=5).tolist() and total == int(p.astype(bool).sum())
    assert np.all(bi % 5 == np.arange(5)) and np.all(bv > 0)


def test_errors(pkg):
    import torch
    m = pkg.generate_matrix(20_000, 1024, 20, "gamma", 4)
    x = pkg.create_sample_vector(1024, True, False, True, 2)
    dthr = torch.full((4,), 0.5, dtype=torch.float32, device="cuda")
    dcnt = torch.zeros((4 * 16,), dtype=torch.int32, device="cuda")
    dbest = torch.zeros((4 * 16 + 1,), dtype=torch.int64, device="cuda")
    dtot = torch.zeros((4,), dtype=torch.int32, device="cuda")
    dlab = torch.zeros((20_000,), dtype=torch.int32, device="cuda")
    dxs = torch.from_numpy(np.tile(x, (4, 1))).cuda()
    torch.cuda.synchronize()
    T, N, B, S, L, X = dthr.data_ptr(), dcnt.data_ptr(), dbest.data_ptr(), dtot.data_ptr(), dlab.data_ptr(), dxs.data_ptr()

    def status_of(fn):
        with pytest.raises(pkg.TkspmvError) as e:
            fn()
        return e.value.status

    for kw in (dict(precision=pkg.F16), dict(partitions=4, k_per_partition=8)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, **kw)
        eng.reset(x)
        eng.set_groups(np.zeros(m.rows, dtype=np.uint32), 1)
        assert status_of(lambda: eng.enqueue_facets(0, 1, T, N, 16, L)) == pkg._lib.ERR_UNSUPPORTED, kw
        assert status_of(lambda: eng.run_facets(0.5)) == pkg._lib.ERR_UNSUPPORTED, kw
        eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    ST, INV = pkg._lib.ERR_STATE, pkg._lib.ERR_INVALID
    assert status_of(lambda: eng.enqueue_facets(0, 1, T, N, 16, L)) == ST                    # no query vector installed
    assert status_of(lambda: eng.run_facets(0.5)) == ST
    eng.reset(x)
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, N)) == ST                           # no labels installed
    assert status_of(lambda: eng.run_facets(0.5)) == ST
    assert status_of(lambda: eng.enqueue_facets(X, 0, T, N, 16, L)) == INV                   # count < 1
    assert status_of(lambda: eng.enqueue_facets(X, 1, 0, N, 16, L)) == INV                   # no thresholds
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, 0, 16, L)) == INV                   # no counts
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, N, 16, L, mask_stride=-1)) == INV   # negative stride
    assert status_of(lambda: eng.enqueue_facets(0, 2, T, N, 16, L)) == INV                   # the installed vector: count must be 1
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, N, 0, L)) == INV                    # labels with n_bins = 0
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, N, 16, 0)) == INV                   # n_bins without labels
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, N, (1 << 30) + 1, L)) == INV        # n_bins > 2^30
    assert status_of(lambda: eng.enqueue_facets(X, 1, T, N, 16, L, B + 4)) == INV            # dev_best not 8-byte aligned
    lib = pkg._lib.lib()
    tot = C.c_uint64(0)
    eng.set_groups(np.zeros(m.rows, dtype=np.uint32), 1)
    assert lib.tkspmv_run_facets(eng._h, 0.5, 1, None, None, C.byref(tot)) == INV            # use_filter, none installed
    # and the valid forms of the same calls go through
    eng.enqueue_facets(X, 4, T, N, 16, L, B, S)
    eng.enqueue_facets(0, 1, T, N, 16, L)
    eng.enqueue_facets(0, 1, T, N)
    eng.synchronize()
    assert lib.tkspmv_run_facets(eng._h, 0.5, 0, None, None, None) == pkg._lib.OK
    eng.close()
