"""Nearest-n assignment (tkspmv_enqueue_nearest / tkspmv_nearest; SpMV.enqueue_nearest, nearest, nearest_spmv) on the MI355X.

Everything is compared bit for bit. The expectation is the host twin, Packed.nearest of a Packed built with the engine's own geometry
-- which test_nearest_host.py pins to host.nearest_n over the order-matched oracle's scores of the whole stream --, so values and
vectors are signed and general. The counts straddle the vectors one pass holds (16 / 4 / 1 at 1024 / 4096 / 16384 columns) and the
list length: the launches behind the first merge with the stored lists. On top: ties inside a pass and across passes, the identity
with enqueue_assign and with the scoring path of the same engine, the masks (one made by enqueue_match in stream order), the
composition with enqueue_label_sums, guard zones on both streams, the engine state a pass must not touch, and the status codes.
The conftest syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import bits, coo, signed
from test_score_rows_host import _hand_made

pytestmark = pytest.mark.gpu

GUARD = 64
NS = (1, 2, 3, 4)
NONE = 0xFFFFFFFF
SENT = -7


def _xs(count, cols, seed):
    return np.random.default_rng(seed).standard_normal((count, cols)).astype(np.float32)


def _packed_like(pkg, eng, m):
    info = eng.info()
    packed = pkg.Packed(m, k=eng.k, nnz_per_lane=info["packet_entries"] // 64, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    return packed


def _same(got, want, label):
    (gl, gs), (wl, ws) = got, want
    assert gl.dtype == np.uint32 and gs.dtype == np.float32 and gl.shape == gs.shape == wl.shape, label
    bad = np.flatnonzero(np.any((gl != wl) | (bits(gs) != bits(ws)), axis=1))
    assert bad.size == 0, f"{label}: {bad.size} rows differ from the host twin, first {bad[:4]}: {gl[bad[:4]].tolist()} / {gs[bad[:4]].tolist()} != {wl[bad[:4]].tolist()} / {ws[bad[:4]].tolist()}"


def _check_engine(pkg, eng, m, xs, n, label, packed=None, mask=None):
    """eng.nearest(xs, n, mask) == the host twin on the engine's own layout, labels and score bits."""
    packed = _packed_like(pkg, eng, m) if packed is None else packed
    got = eng.nearest(xs, n, mask)
    assert got[0].shape == (m.rows, n), label
    _same(got, packed.nearest(xs, n, mask), label)
    return got


GENERATED = [(300, 4, (1, 2, 3, 4, 5, 15, 16, 17, 33)), (1024, 4, (1, 2, 3, 4, 5, 15, 16, 17, 33)), (1024, 8, (1, 2, 3, 4, 5, 15, 16, 17, 33)),
             (4096, 4, (1, 4, 5, 9)), (16384, 4, (1, 3, 5))]


@pytest.mark.parametrize("cols,c_lane,counts", GENERATED)
def test_generated_matrices(pkg, cols, c_lane, counts):
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, "gamma" if cols == 1024 else "uniform", 5 + cols), cols)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, nnz_per_lane=c_lane)
    assert eng.info()["packet_entries"] == 64 * c_lane
    packed = _packed_like(pkg, eng, m)
    xs = _xs(max(counts), cols, 300 + cols)
    for count in counts:
        for n in NS:
            labels, _ = _check_engine(pkg, eng, m, xs[:count], n, f"2500x{cols} C={c_lane} count={count} n={n}", packed)
            if n == 1:
                assert len(set(labels[:, 0].tolist())) == count, (cols, count)  # every vector wins somewhere: the later passes' merges show
    eng.close()


@pytest.mark.parametrize("c_lane", [4, 8])
def test_hand_made_rows(pkg, c_lane):
    """Empty rows in front, in the middle and at the end; rows of 256, 512 and 1500 entries, which span packets: a carry per vector."""
    m, lens = _hand_made(pkg, 1024)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
    xs = _xs(17, 1024, 11)
    empty = [r for r in range(m.rows) if r not in lens]
    half = np.arange(m.rows) % 2 == 0
    for count in (3, 17):
        for n in NS:
            labels, scores = _check_engine(pkg, eng, m, xs[:count], n, f"hand-made C={c_lane} count={count} n={n}")
            k = min(n, count)
            assert np.all(labels[empty][:, :k] == np.arange(k, dtype=np.uint32)) and np.all(bits(scores[empty][:, :k]) == 0)
            assert np.all(labels[empty][:, k:] == NONE) and np.all(scores[empty][:, k:] == -np.inf)
            _check_engine(pkg, eng, m, xs[:count], n, f"hand-made C={c_lane} count={count} n={n} masked", mask=half)
    eng.close()


def test_partition_tails(pkg):
    rng = np.random.default_rng(7)
    rows, per = 128, 8  # 1024 entries: rows end on the last slot of a packet
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    xs = _xs(17, 512, 8)
    for c_lane in (4, 8):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
        for n in (2, 4):
            _check_engine(pkg, eng, m, xs, n, f"exact fit C={c_lane} n={n}")
        eng.close()


def test_from_packed_first_row_approximate_and_geometry(pkg, tmp_path):
    m = signed(pkg, pkg.generate_matrix(6000, 1024, 20, "gamma", 9), 9)
    xs = _xs(17, 1024, 10)
    # an engine made from a saved and loaded file: no COO anywhere near it
    hint = pkg.Packed.wave_partitions(device=0, m=m)
    packed = pkg.Packed(m, k=16, n_wave_partitions=hint)
    packed.save(tmp_path / "m.tkspmv")
    eng = pkg.SpMV.from_packed(pkg.Packed.load(tmp_path / "m.tkspmv"), k=16, device=0)
    plain_labels, _ = _check_engine(pkg, eng, m, xs, 3, "from_packed", packed)
    eng.close()
    # first_row: the outputs and the mask are indexed by LOCAL row and the labels are unaffected
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, first_row=1000)
    labels, _ = _check_engine(pkg, eng, m, xs, 3, "first_row=1000")
    assert np.array_equal(labels, plain_labels) or eng.info()["n_wave_partitions"] != hint
    _check_engine(pkg, eng, m, xs, 2, "first_row=1000 masked", mask=np.arange(m.rows) % 3 == 0)
    eng.close()
    # an approximate per-partition engine is served (without a mask: masks share the filtered queries' scope)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    _check_engine(pkg, eng, m, xs, 4, "partitions=8")
    eng.close()
    # off the default launch geometry: the kernel always launches 512 threads over the engine's grid and partition table
    for kw in (dict(threads_per_wg=256, waves_per_cu=4), dict(threads_per_wg=64, waves_per_cu=4), dict(waves_per_cu=1)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, **kw)
        _check_engine(pkg, eng, m, xs, 4, f"geometry {kw}")
        eng.close()


def test_long_partitions(pkg):
    """8 partitions of several hundred packets each (the shape of test_gpu_long_partitions.py): a wave walks them all, every
    vector's carry with it."""
    m = signed(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41)
    packed = pkg.Packed(m, k=16, n_wave_partitions=8)
    assert packed.info()["packets_per_partition"] >= 300
    eng = pkg.SpMV.from_packed(packed, k=16, device=0)
    assert eng.info()["n_wave_partitions"] == 8
    _check_engine(pkg, eng, m, _xs(5, 1024, 42), 4, "8 long partitions", packed)
    eng.close()


def test_ties_within_and_across_passes(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 13), 13)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    packed = _packed_like(pkg, eng, m)
    xs = _xs(20, 1024, 14)
    # a duplicate follows its original directly and never precedes it: inside one pass (3 = 0) and across two passes (17 = 2)
    for dup_at, orig in ((3, 0), (17, 2)):
        dup = xs.copy()
        dup[dup_at] = dup[orig]
        for n in (2, 4):
            labels, scores = _check_engine(pkg, eng, m, dup, n, f"duplicate {dup_at} = {orig} n={n}", packed)
            ro, jo = np.nonzero(labels == orig)
            inside = jo < n - 1
            assert ro.size > 0 and np.all(labels[ro[inside], jo[inside] + 1] == dup_at)
            assert np.array_equal(bits(scores[ro[inside], jo[inside] + 1]), bits(scores[ro[inside], jo[inside]]))
            rd, jd = np.nonzero(labels == dup_at)
            assert np.all(jd > 0) and np.all(labels[rd, jd - 1] == orig)
    # all-zero vectors: labels 0 .. n-1 with +0.0f in every row, in one pass and in two
    for count in (3, 20):
        for n in NS:
            l0, s0 = eng.nearest(np.zeros((count, 1024), dtype=np.float32), n)
            k = min(n, count)
            assert np.all(l0[:, :k] == np.arange(k, dtype=np.uint32)) and np.all(bits(s0[:, :k]) == 0), (count, n)
    # x and -x: rows whose score is a zero of either sign tie, label 0 first (rows of one entry in a column where x is zero)
    one = coo(pkg, 64, 1024, np.arange(64), np.arange(64), np.ones(64))
    x = xs[0].copy()
    x[:32] = 0.0
    e1 = pkg.SpMV(one.row, one.col, one.val, one.rows, one.cols, k=4, device=0)
    lz, sz = _check_engine(pkg, e1, one, np.stack([x, -x]), 2, "x and -x")
    assert np.all(lz[:32] == np.array([0, 1], dtype=np.uint32)) and np.all(sz[:32] == 0)
    e1.close()
    eng.close()


def test_column_consistency(pkg):
    """Column 0 of n = 4 is enqueue_assign's answer, n = 1 is it exactly; every listed score is what score_rows reports for that row
    and vector on the same engine, and the lists are nearest_n of score_rows' scores."""
    import torch
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 17), 17)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, first_row=500)
    xs = _xs(20, 1024, 18)
    a_lab, a_best = eng.assign(xs)
    for n in (1, 4):
        labels, scores = eng.nearest(xs, n)
        assert np.array_equal(labels[:, 0], a_lab) and np.array_equal(bits(scores[:, 0]), bits(a_best)), n
    ids = np.random.default_rng(3).choice(m.rows, 200, replace=False).astype(np.uint32)
    all_scores = eng.score_rows(ids + np.uint32(500), xs)  # [20, 200]
    want_l, want_s = pkg.nearest_n(all_scores, 4)
    assert np.array_equal(want_l, labels[ids]) and np.array_equal(bits(want_s), bits(scores[ids]))
    picked = np.take_along_axis(all_scores.T, labels[ids].astype(np.int64), axis=1)  # scores[r][j] == score_rows([r], xs[labels[r][j]])
    assert np.array_equal(bits(picked), bits(scores[ids]))
    assert np.all(pkg.margin(scores) >= 0)
    eng.close()


def test_masks(pkg):
    import torch
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 33), 33)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    packed = _packed_like(pkg, eng, m)
    xs = _xs(20, 1024, 34)
    rng = np.random.default_rng(35)
    one = np.zeros(m.rows, dtype=bool)
    one[m.rows // 2] = True
    for n in (1, 3, 4):
        for count in (6, 20):
            plain = _check_engine(pkg, eng, m, xs[:count], n, f"plain n={n} count={count}", packed)
            _same(eng.nearest(xs[:count], n, np.ones(m.rows, dtype=bool)), plain, "all ones")
            for name, mask in (("half", rng.random(m.rows) < 0.5), ("one row", one), ("none", np.zeros(m.rows, dtype=bool))):
                labels, scores = _check_engine(pkg, eng, m, xs[:count], n, f"{name} n={n} count={count}", packed, mask)
                assert np.all(labels[~mask] == NONE) and np.all(scores[~mask] == -np.inf), (name, n)
                assert np.array_equal(labels[mask], plain[0][mask]) and np.array_equal(bits(scores[mask]), bits(plain[1][mask])), (name, n)
    # mask = True: the installed filter, whatever installed it
    half = rng.random(m.rows) < 0.5
    eng.set_filter(pkg.row_mask(m.rows, half))
    _same(eng.nearest(xs, 2, True), packed.nearest(xs, 2, half), "installed filter")
    # a mask made on the device by enqueue_match, consumed in stream order without a host round trip
    clauses, pred = pkg.bool_query(m.cols, should=[range(0, 300)], min_should=1)
    want_mask = pkg.match_rows(m.row, m.col, m.rows, clauses, pred)
    assert 0 < np.count_nonzero(want_mask) < m.rows
    dt = torch.from_numpy(clauses.view(np.int32).copy()).cuda()
    dp = torch.from_numpy(np.array([int(v) & 0xFFFFFFFF for v in pred], dtype=np.uint32).view(np.int32)).cuda()
    dmask = torch.zeros((m.rows + 31) // 32, dtype=torch.int32, device="cuda")
    d_xs = torch.from_numpy(xs).cuda()
    d_lab = torch.full((m.rows, 3), SENT, dtype=torch.int32, device="cuda")
    d_sc = torch.full((m.rows, 3), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_match(dt.data_ptr(), dp.data_ptr(), 1, dmask.data_ptr())
    eng.enqueue_nearest(d_xs.data_ptr(), 20, 3, d_lab.data_ptr(), d_sc.data_ptr(), dev_mask=dmask.data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    _same((d_lab.cpu().numpy().view(np.uint32), d_sc.cpu().numpy()), packed.nearest(xs, 3, want_mask), "mask from enqueue_match")
    eng.close()


def test_composition_with_label_sums(pkg):
    """nearest(n = 1, mask) -> enqueue_label_sums(n_bins = count): the rows outside the mask carry NONE and fall into no bin."""
    import torch
    m = signed(pkg, pkg.generate_matrix(5000, 1024, 20, "gamma", 43), 43)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    count = 12
    xs = _xs(count, 1024, 44)
    mask = np.random.default_rng(45).random(m.rows) < 0.4
    d_xs = torch.from_numpy(xs).cuda()
    d_mask = torch.from_numpy(pkg.row_mask(m.rows, mask).view(np.int32).copy()).cuda()
    d_lab = torch.zeros(m.rows, dtype=torch.int32, device="cuda")
    d_sc = torch.zeros(m.rows, dtype=torch.float32, device="cuda")
    d_sums = torch.zeros((count, m.cols), dtype=torch.int64, device="cuda")
    e = eng.sums_exponent()
    torch.cuda.synchronize()
    eng.enqueue_nearest(d_xs.data_ptr(), count, 1, d_lab.data_ptr(), d_sc.data_ptr(), dev_mask=d_mask.data_ptr())
    eng.enqueue_label_sums(d_lab.data_ptr(), count, e, d_sums.data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    labels = d_lab.cpu().numpy().view(np.uint32)
    want_l = np.where(mask, eng.assign(xs)[0], np.uint32(NONE)).astype(np.uint32)
    assert np.array_equal(labels, want_l)
    assert np.array_equal(d_sums.cpu().numpy(), pkg.label_sums(m, want_l, count, e))
    eng.close()


def test_enqueue_into_guarded_buffers(pkg):
    """Exactly rows * n labels and scores change: guard zones of 64 words on both sides of both outputs keep their sentinel, on the
    engine's stream and on a caller's stream, with and without a mask."""
    import torch
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 31), 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, first_row=77)
    xs = _xs(33, 1024, 32)
    d_xs = torch.from_numpy(xs).cuda()
    packed = _packed_like(pkg, eng, m)
    mask = np.arange(m.rows) % 3 != 1
    d_mask = torch.from_numpy(pkg.row_mask(m.rows, mask).view(np.int32).copy()).cuda()
    side = torch.cuda.Stream()
    for count, n, masked in ((16, 3, False), (33, 1, False), (33, 4, True), (5, 2, True)):
        want_l, want_s = packed.nearest(xs[:count], n, mask if masked else None)
        for stream in (None, side):
            lab = torch.empty(GUARD + m.rows * n + GUARD, dtype=torch.int32, device="cuda")
            sc = torch.empty(GUARD + m.rows * n + GUARD, dtype=torch.float32, device="cuda")
            args = (d_xs.data_ptr(), count, n, lab.data_ptr() + 4 * GUARD, sc.data_ptr() + 4 * GUARD, d_mask.data_ptr() if masked else 0)
            if stream is None:
                lab.fill_(SENT), sc.fill_(SENT)
                torch.cuda.synchronize()  # torch's fills are complete before the engine's stream starts
                eng.enqueue_nearest(*args)
                eng.synchronize()
            else:
                with torch.cuda.stream(side):
                    lab.fill_(SENT), sc.fill_(SENT)  # the fills run on the caller's stream, in front of the passes
                eng.enqueue_nearest(*args, stream=side.cuda_stream)
                done = torch.cuda.Event()
                done.record(side)
                done.synchronize()
            hl, hs = lab.cpu().numpy(), sc.cpu().numpy()
            assert np.all(hl[:GUARD] == SENT) and np.all(hl[GUARD + m.rows * n:] == SENT), "labels written outside [0, rows * n)"
            assert np.all(hs[:GUARD] == SENT) and np.all(hs[GUARD + m.rows * n:] == SENT), "scores written outside [0, rows * n)"
            got = (hl[GUARD:GUARD + m.rows * n].view(np.uint32).reshape(m.rows, n), hs[GUARD:GUARD + m.rows * n].reshape(m.rows, n))
            _same(got, (want_l, want_s), f"count={count} n={n} masked={masked} side={stream is not None}")
    eng.close()


def test_engine_state_is_untouched(pkg):
    import torch
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    d_q = torch.from_numpy(xq).cuda()
    d_xs = torch.from_numpy(_xs(20, 1024, 22)).cuda()
    d_lab = torch.zeros((m.rows, 4), dtype=torch.int32, device="cuda")
    d_sc = torch.zeros((m.rows, 4), dtype=torch.float32, device="cuda")
    d_idx = [torch.zeros((8, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    d_val = [torch.zeros((8, k), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    # the reference: a batch call alone
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[0].data_ptr(), d_val[0].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    want_idx, want_val = d_idx[0].cpu().numpy().copy(), bits(d_val[0].cpu().numpy()).copy()
    eng.enqueue_batch(d_q.data_ptr(), 8)  # (engine-owned result pair: the last query wins)
    eng.synchronize()
    res0, counters0 = eng.read_result(), eng.debug_counters()
    eng.enqueue_nearest(d_xs.data_ptr(), 20, 4, d_lab.data_ptr(), d_sc.data_ptr())
    eng.enqueue_nearest(d_xs.data_ptr(), 5, 2, d_lab.data_ptr(), d_sc.data_ptr())
    eng.synchronize()
    res1, counters1 = eng.read_result(), eng.debug_counters()
    assert counters1 == counters0, "enqueue_nearest moved a counter"
    assert np.array_equal(res0[1], res1[1]) and np.array_equal(bits(res0[0]), bits(res1[0])), "enqueue_nearest changed the result pair"
    # a batch call right behind an unwaited call returns the same lists
    d_idx[1].zero_(), d_val[1].zero_()
    torch.cuda.synchronize()
    eng.enqueue_nearest(d_xs.data_ptr(), 20, 4, d_lab.data_ptr(), d_sc.data_ptr())
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[1].data_ptr(), d_val[1].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_idx[1].cpu().numpy(), want_idx) and np.array_equal(bits(d_val[1].cpu().numpy()), want_val)
    eng.close()


def test_status_codes(pkg):
    import torch
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    d_lab = torch.full((m.rows, 4), SENT, dtype=torch.int32, device="cuda")
    d_sc = torch.full((m.rows, 4), SENT, dtype=torch.float32, device="cuda")
    xs = _xs(17, 512, 62)
    d_xs = torch.from_numpy(xs).cuda()
    d_mask = torch.from_numpy(pkg.row_mask(m.rows).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    INVALID, UNSUPPORTED, STATE = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED, pkg._lib.ERR_STATE
    lib, X, Lb, S, M = pkg._lib.lib(), d_xs.data_ptr(), d_lab.data_ptr(), d_sc.data_ptr(), d_mask.data_ptr()
    h_lab = np.full((m.rows, 4), SENT, dtype=np.int32)
    h_sc = np.full((m.rows, 4), SENT, dtype=np.float32)
    HX, HL, HS = xs.ctypes.data_as(C.POINTER(C.c_float)), h_lab.ctypes.data_as(C.POINTER(C.c_uint32)), h_sc.ctypes.data_as(C.POINTER(C.c_float))

    def status_of(fn):
        try:
            fn()
        except pkg.TkspmvError as e:
            return e.status
        return 0

    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=prec)
        assert status_of(lambda: eng.enqueue_nearest(X, 2, 2, Lb, S)) == UNSUPPORTED, prec
        assert status_of(lambda: eng.nearest(xs, 2)) == UNSUPPORTED, prec
        assert lib.tkspmv_nearest(eng._h, HX, 2, 2, 0, HL, HS) == UNSUPPORTED, prec
        assert lib.tkspmv_nearest(eng._h, HX, 2, 2, 1, HL, HS) == UNSUPPORTED, prec  # (before STATE)
        assert status_of(lambda: eng.enqueue_nearest(X, 0, 2, Lb, S)) == INVALID, prec  # INVALID comes before UNSUPPORTED
        assert status_of(lambda: eng.enqueue_nearest(X, 2, 5, Lb, S)) == INVALID, prec
        assert status_of(lambda: eng.enqueue_nearest(X, 2, 2, 0, S)) == INVALID, prec
        assert status_of(lambda: eng.enqueue_nearest(X, 2, 2, Lb, 0)) == INVALID, prec
        assert status_of(lambda: eng.enqueue_nearest(0, 2, 2, Lb, S)) == INVALID, prec
        eng.close()
    # an approximate per-partition engine: served without a mask, UNSUPPORTED with one (where col_stats with a mask is)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    masked_cs = status_of(lambda: eng.enqueue_col_stats(pkg._lib.COL_NNZ, torch.zeros(m.cols, dtype=torch.int32, device="cuda").data_ptr(), masks=M))
    assert status_of(lambda: eng.enqueue_nearest(X, 2, 2, Lb, S, dev_mask=M)) == masked_cs
    eng.synchronize()
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    for count in (0, -1):
        assert status_of(lambda: eng.enqueue_nearest(X, count, 2, Lb, S)) == INVALID, count
        assert lib.tkspmv_nearest(eng._h, HX, count, 2, 0, HL, HS) == INVALID, count
    for n in (0, -1, 5):
        assert status_of(lambda: eng.enqueue_nearest(X, 2, n, Lb, S)) == INVALID, n
        assert lib.tkspmv_nearest(eng._h, HX, 2, n, 0, HL, HS) == INVALID, n
    assert status_of(lambda: eng.enqueue_nearest(0, 2, 2, Lb, S)) == INVALID
    assert status_of(lambda: eng.enqueue_nearest(X, 2, 2, 0, S)) == INVALID
    assert status_of(lambda: eng.enqueue_nearest(X, 2, 2, Lb, 0)) == INVALID
    assert lib.tkspmv_nearest(eng._h, None, 2, 2, 0, HL, HS) == INVALID and lib.tkspmv_nearest(eng._h, HX, 2, 2, 0, None, HS) == INVALID
    assert lib.tkspmv_nearest(eng._h, HX, 2, 2, 1, HL, HS) == STATE  # use_filter without an installed filter
    assert status_of(lambda: eng.nearest(xs, 2, True)) == STATE
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(h_lab == SENT) and np.all(h_sc == SENT), "a rejected call wrote its host output"
    assert np.all(d_lab.cpu().numpy() == SENT) and np.all(d_sc.cpu().numpy() == SENT), "a rejected call wrote its device output"
    # what is allowed works: the host form without host_scores writes rows * n labels and nothing else
    want_l, _ = _packed_like(pkg, eng, m).nearest(xs, 3)
    assert lib.tkspmv_nearest(eng._h, HX, 17, 3, 0, HL, None) == 0
    flat = h_lab.reshape(-1)
    assert np.array_equal(flat[:m.rows * 3].view(np.uint32).reshape(m.rows, 3), want_l) and np.all(flat[m.rows * 3:] == SENT) and np.all(h_sc == SENT)
    with pytest.raises(ValueError):
        eng.nearest(xs[:, :-1], 2)
    eng.close()
    # (rows = 0 cannot be reached through an engine: tkspmv_create refuses a matrix without entries)


def test_one_shot_helper(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 71), 71)
    xs = _xs(6, 1024, 72)
    mask = np.arange(m.rows) % 2 == 0
    labels, scores = pkg.nearest_spmv(m, xs, 2, mask, device=0)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    _same((labels, scores), eng.nearest(xs, 2, mask), "nearest_spmv")
    eng.close()


def test_host_forms_interleaved_on_one_engine(pkg):
    """nearest and assign in turn on ONE engine, each call with another list length and another number of vectors -- the smallest
    sequence in which result arrays sized for one n, or a vector chunk sized for one count, are used again for another. Rows without
    entries, rows on which every vector ties and rows outside the mask are among the 300."""
    rng = np.random.default_rng(81)
    rows, cols, per = 300, 1024, 6
    keep = np.ones(rows, dtype=bool)
    keep[[0, 7, 150, 299]] = False  # rows without entries: the first, the last, two in between
    tied = np.arange(10, 15)  # one entry each, in column 0, where every vector holds 1.0
    keep[tied] = False
    r = np.repeat(np.flatnonzero(keep), per)
    r, c, v = np.concatenate([r, tied]), np.concatenate([rng.integers(1, cols, r.size), np.zeros(tied.size)]), np.concatenate([rng.standard_normal(r.size), np.full(tied.size, 0.5)])
    by_row = np.argsort(r, kind="stable")
    m = coo(pkg, rows, cols, r[by_row], c[by_row], v[by_row])
    xs = _xs(40, cols, 82)
    xs[:, 0] = 1.0
    xs[35] = xs[1]  # a tie across passes
    mask = np.ones(rows, dtype=bool)
    mask[[7, 12, 20]] = False  # an empty row, a tied row and an ordinary one
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0)
    packed = _packed_like(pkg, eng, m)

    def assign(count, label):
        (gl, gb), (wl, wb) = eng.assign(xs[:count]), packed.assign(xs[:count])
        _same((gl[:, None], gb[:, None]), (wl[:, None], wb[:, None]), label)
        return gl

    labels, _ = _check_engine(pkg, eng, m, xs[:3], 4, "nearest(n=4), 3 vectors", packed)
    assert np.all(labels[tied] == np.array([0, 1, 2, NONE], dtype=np.uint32)) and np.all(labels[0] == labels[tied[0]])
    a40 = assign(40, "assign, 40 vectors: three passes")
    assert np.all(a40[tied] == 0) and not np.any(a40 == 35) and np.any(a40 == 1) and np.any(a40 > 31)
    labels, _ = _check_engine(pkg, eng, m, xs[:17], 2, "nearest(n=2, mask), 17 vectors", packed, mask)
    assert np.all(labels[~mask] == NONE) and np.all(labels[11] == np.array([0, 1], dtype=np.uint32))
    assert np.all(assign(1, "assign, 1 vector") == 0)
    labels, _ = _check_engine(pkg, eng, m, xs, 1, "nearest(n=1), 40 vectors", packed)
    assert np.array_equal(labels[:, 0], a40)
    eng.close()


def test_host_forms_across_the_vector_chunk(pkg):
    """One vector more than the host forms upload at once (64 MiB: 1024 vectors of 16384 columns): the second chunk holds vector 1024
    alone, which merges with the first chunk's results as vector 1024. It is a copy of vector 3, so a tie crosses the chunk
    boundary and goes to 3."""
    rng = np.random.default_rng(91)
    rows, cols, per, count = 96, 16384, 5, 1025
    m = coo(pkg, rows, cols, np.repeat(np.arange(rows), per), rng.integers(0, cols, rows * per), rng.standard_normal(rows * per))
    xs = rng.standard_normal((count, cols), dtype=np.float32)
    xs[3] *= 8.0  # the best vector of many rows ...
    xs[1024] = xs[3]  # ... and its copy behind the boundary
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0)
    packed = _packed_like(pkg, eng, m)
    (gl, gb), (wl, wb) = eng.assign(xs), packed.assign(xs)
    _same((gl[:, None], gb[:, None]), (wl[:, None], wb[:, None]), "assign, 1025 vectors")
    assert np.count_nonzero(gl == 3) >= 8 and not np.any(gl == 1024)
    labels, _ = _check_engine(pkg, eng, m, xs, 2, "nearest(n=2), 1025 vectors", packed)
    assert np.array_equal(labels[:, 0], gl) and np.all(labels[gl == 3, 1] == 1024) and np.all(labels[labels[:, 1] == 1024, 0] == 3)
    eng.close()
