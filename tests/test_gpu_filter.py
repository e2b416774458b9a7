"""Filtered top-k (tkspmv_enqueue_filtered / tkspmv_set_filter) on the MI355X.

Every result is checked BIT FOR BIT against the order-matched oracle restricted to the allowed rows
(oracle.select_topk(packed_scores, present & allow, k, min_score, first_row), the bit-exact leg of test_gpu_parity.py), and the
queries with min_score 0 also against the independent gold leg (fp64 scores from the COO, restricted to the same rows).
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import numpy as np
import pytest

import support
from support import Scores

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _engine(pkg, m, k, **kw):
    return pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, **kw)


def _packed_scores(pkg, oracle, eng, m, x):
    return Scores(pkg, eng, m)(oracle, x)


def _expect(oracle, yp, present, allow, k, min_score=0.0, first_row=0):
    return oracle.select_topk(yp, (present & allow).astype(np.uint8), k, min_score, first_row)


def _check(oracle, m, x, k, allow, idx, val, ei, ev, min_score=0.0, first_row=0):
    assert np.array_equal(idx, ei), "index list differs from the order-matched oracle restricted to the allowed rows"
    assert np.array_equal(val.view(np.uint32), ev.view(np.uint32)), "scores are not bit-identical"
    if min_score != 0.0:
        return
    # gold leg: fp64 scores from the COO, top-k among the allowed rows that have entries
    y64, present = oracle.scores_f64(m.row, m.col, m.val, x, m.rows)
    elig = np.flatnonzero(present.astype(bool) & allow)
    n = min(k, elig.size)
    assert np.all(idx[n:] == 0) and np.all(val[n:] == 0.0), "fewer than k eligible rows: the tail must be (0, 0.0)"
    if n == 0:
        return
    gold = elig[np.argsort(-y64[elig], kind="stable")[:n]]
    got = idx[:n].astype(np.int64) - first_row
    kth = y64[gold[-1]]
    for r in set(got.tolist()) ^ set(gold.tolist()):
        assert abs(y64[r] - kth) <= 2e-6 * max(abs(kth), 1e-30), f"row {r} is not a boundary tie"
    assert np.all(allow[got]), "a masked row was returned"
    assert np.allclose(np.sort(val[:n])[::-1], np.sort(y64[gold])[::-1], rtol=RTOL, atol=0)


@pytest.mark.parametrize("rows,cols,nnz,k,kw", [
    (1_000_000, 1024, 20, 100, {}),                 # deferred selection chain
    (200_000, 4096, 20, 100, {}),
    (30_000, 16384, 20, 100, {}),
    (1000, 512, 20, 100, {}),                       # scores + radix select
    (200_000, 1024, 20, 100, {"nnz_per_lane": 8}),
    (100_000, 1024, 20, 100, {"first_row": 5000}),
], ids=["1Mx1024", "200kx4096", "30kx16384", "1000x512_radix", "c8", "first_row"])
def test_filtered_matches_oracle(pkg, oracle, rows, cols, nnz, k, kw):
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", rows % 97 + 3)
    x = pkg.create_sample_vector(cols, True, False, True, 17)
    first_row = kw.get("first_row", 0)
    eng = _engine(pkg, m, k, **kw)
    yp, present = _packed_scores(pkg, oracle, eng, m, x)
    # all-ones mask: exactly the unfiltered exact result of the same engine
    eng.reset(x)
    eng()
    uv, ui = eng.read_result()
    fv, fi = eng.run_filtered(allow=np.ones(rows, dtype=bool))
    assert np.array_equal(fi, ui) and np.array_equal(fv.view(np.uint32), uv.view(np.uint32))
    ei, ev = _expect(oracle, yp, present, np.ones(rows, dtype=bool), k, 0.0, first_row)
    _check(oracle, m, x, k, np.ones(rows, dtype=bool), fi, fv, ei, ev, 0.0, first_row)
    masks = support.masks(rows, ui, first_row, rows)
    for name, allow in masks.items():
        val, idx = eng.run_filtered(allow=allow)
        ei, ev = _expect(oracle, yp, present, allow, k, 0.0, first_row)
        _check(oracle, m, x, k, allow, idx, val, ei, ev, 0.0, first_row)
    eng.close()
    # a positive min_score (an engine parameter): about the 30th best unfiltered score, so the sparse masks keep fewer than k rows
    ms = float(uv[min(29, k - 1)])
    eng = _engine(pkg, m, k, min_score=ms, **kw)
    eng.reset(x)
    for name, allow in masks.items():
        val, idx = eng.run_filtered(allow=allow)
        ei, ev = _expect(oracle, yp, present, allow, k, ms, first_row)
        _check(oracle, m, x, k, allow, idx, val, ei, ev, ms, first_row)
    eng.close()


@pytest.fixture(scope="module")
def big(pkg, oracle):
    m = pkg.generate_matrix(1_000_000, 1024, 20, "gamma", 41)
    x = pkg.create_sample_vector(1024, True, False, True, 23)
    eng = _engine(pkg, m, 100)
    yp, present = _packed_scores(pkg, oracle, eng, m, x)
    eng.reset(x)
    yield m, x, eng, yp, present
    eng.close()


def test_degenerate_masks(pkg, oracle, big):
    m, x, eng, yp, present = big
    rows, k = m.rows, eng.k
    cases = {}
    block = np.zeros(rows, dtype=bool)
    block[400_000:400_500] = True  # one contiguous block, far smaller than k threshold groups' worth of rows
    cases["block"] = block
    few = np.zeros(rows, dtype=bool)
    few[np.random.default_rng(5).choice(rows, 30, replace=False)] = True  # fewer than k eligible rows
    cases["few"] = few
    cases["none"] = np.zeros(rows, dtype=bool)
    for name, allow in cases.items():
        val, idx = eng.run_filtered(allow=allow)
        ei, ev = _expect(oracle, yp, present, allow, k)
        _check(oracle, m, x, k, allow, idx, val, ei, ev)
        if name == "few":
            n = int((present & allow).sum())
            assert n < k and np.all(idx[n:] == 0) and np.all(val[n:] == 0.0)
        if name == "none":
            assert np.all(idx == 0) and np.all(val == 0.0)


def test_per_query_masks(pkg, oracle):
    import torch
    rows, cols, k, nq = 200_000, 1024, 100, 40  # 40 queries: more than one batch launch's worth
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 12)
    eng = _engine(pkg, m, k)
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 300 + i) for i in range(nq)]).astype(np.float32)
    rng = np.random.default_rng(3)
    allows = [rng.random(rows) < (0.5 if i % 3 else 0.02) for i in range(nq)]
    words = np.stack([pkg.row_mask(rows, a) for a in allows])
    wpr = words.shape[1]
    dxs = torch.from_numpy(xs).cuda()
    dmask = torch.from_numpy(words.view(np.int32)).cuda()
    out_i = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_filtered(dxs.data_ptr(), nq, dmask.data_ptr(), wpr, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    gi, gv = out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy()
    expected = []
    sc = Scores(pkg, eng, m)
    for i in range(nq):
        yp, present = sc(oracle, xs[i])
        expected.append((yp, present))
        ei, ev = _expect(oracle, yp, present, allows[i], k)
        _check(oracle, m, xs[i], k, allows[i], gi[i], gv[i], ei, ev)
    # one mask for every query (stride 0), launched on a caller's stream (handle 0 would mean the engine's own)
    out_i.fill_(-1)
    out_v.fill_(-1.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    eng.enqueue_filtered(dxs.data_ptr(), nq, dmask.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    gi, gv = out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy()
    for i in range(nq):
        ei, ev = _expect(oracle, *expected[i], allows[0], k)
        _check(oracle, m, xs[i], k, allows[0], gi[i], gv[i], ei, ev)
    # engine-owned result buffers: the last query wins
    torch.cuda.synchronize()
    eng.enqueue_filtered(dxs.data_ptr(), nq, dmask.data_ptr(), wpr)
    eng.synchronize()
    val, idx = eng.read_result()
    ei, ev = _expect(oracle, *expected[-1], allows[-1], k)
    _check(oracle, m, xs[-1], k, allows[-1], idx, val, ei, ev)
    # the engine-owned mask (set_filter) with dev_mask = NULL and the installed query vector
    eng.reset(xs[7])
    eng.set_filter(words[11])
    eng.enqueue_filtered(0, 1, 0)
    eng.synchronize()
    val, idx = eng.read_result()
    ei, ev = _expect(oracle, *expected[7], allows[11], k)
    _check(oracle, m, xs[7], k, allows[11], idx, val, ei, ev)
    eng.close()


def _sequence(pkg, eng, xs, dxs, filtered, torch):
    """enqueue_batch, (filtered sequence), enqueue_batch, tkspmv_run, enqueue_multi: the results of the unfiltered steps."""
    k, nq = eng.k, 8
    res = {}
    out_i = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    res["batch1"] = (out_i.cpu().numpy().view(np.uint32).copy(), out_v.cpu().numpy().copy())
    if filtered is not None:
        dmask, wpr, fo_i, fo_v = filtered
        torch.cuda.synchronize()
        eng.enqueue_filtered(dxs.data_ptr(), nq, dmask.data_ptr(), wpr, fo_i.data_ptr(), fo_v.data_ptr())
        eng.synchronize()
    out_i.zero_()
    out_v.zero_()
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr() + 4 * 4 * xs.shape[1], nq, out_i.data_ptr(), out_v.data_ptr())  # queries 4 .. 11
    eng.synchronize()
    res["batch2"] = (out_i.cpu().numpy().view(np.uint32).copy(), out_v.cpu().numpy().copy())
    eng.reset(xs[3])
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
    fo_i = torch.zeros((8, k), dtype=torch.int32, device="cuda")
    fo_v = torch.zeros((8, k), dtype=torch.float32, device="cuda")
    eng = _engine(pkg, m, k, multi_q=4)
    got = _sequence(pkg, eng, xs, dxs, (dmask, words.shape[1], fo_i, fo_v), torch)
    counters = eng.debug_counters()
    eng.close()
    ref = _engine(pkg, m, k, multi_q=4)
    _sequence(pkg, ref, xs, dxs, None, torch)
    ref_counters = ref.debug_counters()
    # every result oracle-exact
    scores, sc = {}, Scores(pkg, ref, m)

    def yp_of(i):
        if i not in scores:
            scores[i] = sc(oracle, xs[i])
        return scores[i]
    fi, fv = fo_i.cpu().numpy().view(np.uint32), fo_v.cpu().numpy()
    for q in range(8):
        ei, ev = _expect(oracle, *yp_of(q), allows[q], k)
        _check(oracle, m, xs[q], k, allows[q], fi[q], fv[q], ei, ev)
        ei, ev = oracle.select_topk(*yp_of(q), k)
        assert np.array_equal(got["batch1"][0][q], ei) and np.array_equal(got["batch1"][1][q].view(np.uint32), ev.view(np.uint32))
        ei, ev = oracle.select_topk(*yp_of(4 + q), k)
        assert np.array_equal(got["batch2"][0][q], ei) and np.array_equal(got["batch2"][1][q].view(np.uint32), ev.view(np.uint32))
    ei, ev = oracle.select_topk(*yp_of(3), k)
    assert np.array_equal(got["run"][0], ei) and np.array_equal(got["run"][1].view(np.uint32), ev.view(np.uint32))
    # the multi-query pass sums in its own order (row per lane): the oracle's segmented scores, as smoke() checks it
    y, present = oracle.scores_f32_segmented(m.row, m.col, m.val, xs[5], m.rows)
    ei, ev = oracle.select_topk(y, present, k)
    assert np.array_equal(got["multi"][0], ei) and np.array_equal(got["multi"][1].view(np.uint32), ev.view(np.uint32))
    ref.close()
    # no repair the unfiltered sequence alone would not have run
    for key in ("checks_failed", "late_repairs", "single_repairs"):
        assert counters[key] <= ref_counters[key], (key, counters, ref_counters)


def test_errors(pkg):
    m = pkg.generate_matrix(20_000, 1024, 20, "gamma", 4)
    x = pkg.create_sample_vector(1024, True, False, True, 2)
    allow = np.ones(m.rows, dtype=bool)
    eng = _engine(pkg, m, 100, precision=pkg.Q1_7)
    eng.reset(x)
    with pytest.raises(pkg.TkspmvError) as e:
        eng.run_filtered(allow=allow)
    assert e.value.status == pkg._lib.ERR_UNSUPPORTED
    eng.close()
    eng = _engine(pkg, m, 100, partitions=4, k_per_partition=8)
    eng.reset(x)
    with pytest.raises(pkg.TkspmvError) as e:
        eng.run_filtered(allow=allow)
    assert e.value.status == pkg._lib.ERR_UNSUPPORTED
    eng.close()
    eng = _engine(pkg, m, 100)
    with pytest.raises(pkg.TkspmvError) as e:
        eng.enqueue_filtered(0, 1, 0)  # no mask given, none installed
    assert e.value.status == pkg._lib.ERR_INVALID
    eng.set_filter(pkg.row_mask(m.rows, allow))
    with pytest.raises(pkg.TkspmvError) as e:
        eng.enqueue_filtered(0, 1, 0)  # no query vector installed
    assert e.value.status == pkg._lib.ERR_STATE
    eng.reset(x)
    for bad in (dict(count=0), dict(mask_stride=-1)):
        with pytest.raises(pkg.TkspmvError) as e:
            eng.enqueue_filtered(0, bad.get("count", 1), 0, bad.get("mask_stride", 0))
        assert e.value.status == pkg._lib.ERR_INVALID
    eng.set_filter(None)
    with pytest.raises(pkg.TkspmvError) as e:
        eng.enqueue_filtered(0, 1, 0)  # the installed mask was removed
    assert e.value.status == pkg._lib.ERR_INVALID
    eng.close()
