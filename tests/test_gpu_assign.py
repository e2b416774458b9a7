"""Assignment (tkspmv_enqueue_assign / tkspmv_assign; SpMV.enqueue_assign, assign, assign_spmv) on the MI355X.

Everything is compared bit for bit. The expectation is the host twin, Packed.assign of a Packed built with the engine's own geometry
(test_gpu_row_stats._twin's recipe) -- which test_assign_host.py pins to the order-matched oracle over the whole stream --, so values
and vectors are signed and general. The counts straddle the vectors one pass holds (16 / 4 / 1 at 1024 / 4096 / 16384 columns): the
launches behind the first merge with the stored pair. On top: the rules of the contract, the identity with the scoring path of the
same engine, guard zones on both streams, the engine state a pass must not touch, the status codes, and the labels installed as
groups. The conftest syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import bits, coo, signed
from test_score_rows_host import _hand_made

pytestmark = pytest.mark.gpu

GUARD = 64
PASS = {1024: 16, 4096: 4, 16384: 1}  # vectors per pass by column tier


def _xs(count, cols, seed):
    return np.random.default_rng(seed).standard_normal((count, cols)).astype(np.float32)


def _packed_like(pkg, eng, m):
    info = eng.info()
    packed = pkg.Packed(m, k=eng.k, nnz_per_lane=info["packet_entries"] // 64, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    return packed


def _check_engine(pkg, eng, m, xs, label, packed=None):
    """eng.assign(xs) == the host twin on the engine's own layout, labels and score bits."""
    packed = _packed_like(pkg, eng, m) if packed is None else packed
    want_l, want_b = packed.assign(xs)
    got_l, got_b = eng.assign(xs)
    assert got_l.shape == got_b.shape == (m.rows,) and got_l.dtype == np.uint32 and got_b.dtype == np.float32, label
    bad = np.flatnonzero((got_l != want_l) | (bits(got_b) != bits(want_b)))
    assert bad.size == 0, f"{label}: {bad.size} rows differ from the host twin, first {bad[:8]}: {got_l[bad[:8]]} / {got_b[bad[:8]]} != {want_l[bad[:8]]} / {want_b[bad[:8]]}"
    return got_l, got_b


GENERATED = [(300, 4, (1, 2, 15, 16, 17, 33)), (1024, 4, (1, 2, 15, 16, 17, 33)), (1024, 8, (1, 2, 15, 16, 17, 33)), (4096, 4, (1, 4, 5, 9)), (16384, 4, (1, 3))]


@pytest.mark.parametrize("cols,c_lane,counts", GENERATED)
def test_generated_matrices(pkg, cols, c_lane, counts):
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, "gamma" if cols == 1024 else "uniform", 5 + cols), cols)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, nnz_per_lane=c_lane)
    assert eng.info()["packet_entries"] == 64 * c_lane
    packed = _packed_like(pkg, eng, m)
    xs = _xs(max(counts), cols, 300 + cols)
    for count in counts:
        labels, _ = _check_engine(pkg, eng, m, xs[:count], f"2500x{cols} C={c_lane} count={count}", packed)
        assert len(set(labels.tolist())) == count, (cols, count)  # every vector wins somewhere: the later passes' merges show
    eng.close()


@pytest.mark.parametrize("c_lane", [4, 8])
def test_hand_made_rows(pkg, c_lane):
    """Empty rows in front, in the middle and at the end; rows of 256, 512 and 1500 entries, which span packets: a carry per vector."""
    m, lens = _hand_made(pkg, 1024)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
    xs = _xs(17, 1024, 11)
    empty = [r for r in range(m.rows) if r not in lens]
    for count in (3, 17):
        labels, best = _check_engine(pkg, eng, m, xs[:count], f"hand-made C={c_lane} count={count}")
        assert np.all(labels[empty] == 0) and np.all(bits(best[empty]) == 0)
    eng.close()


def test_partition_tails(pkg):
    rng = np.random.default_rng(7)
    rows, per = 128, 8  # 1024 entries: rows end on the last slot of a packet
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    xs = _xs(17, 512, 8)
    for c_lane in (4, 8):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
        _check_engine(pkg, eng, m, xs, f"exact fit C={c_lane}")
        eng.close()


def test_from_packed_first_row_approximate_and_geometry(pkg, tmp_path):
    m = signed(pkg, pkg.generate_matrix(6000, 1024, 20, "gamma", 9), 9)
    xs = _xs(17, 1024, 10)
    # an engine made from a saved and loaded file: no COO anywhere near it
    hint = pkg.Packed.wave_partitions(device=0, m=m)
    packed = pkg.Packed(m, k=16, n_wave_partitions=hint)
    packed.save(tmp_path / "m.tkspmv")
    eng = pkg.SpMV.from_packed(pkg.Packed.load(tmp_path / "m.tkspmv"), k=16, device=0)
    plain_labels, _ = _check_engine(pkg, eng, m, xs, "from_packed", packed)
    eng.close()
    # first_row: the outputs are indexed by LOCAL row and the labels are unaffected
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, first_row=1000)
    labels, _ = _check_engine(pkg, eng, m, xs, "first_row=1000")
    assert np.array_equal(labels, plain_labels) or eng.info()["n_wave_partitions"] != hint
    eng.close()
    # an approximate per-partition engine is served
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    _check_engine(pkg, eng, m, xs, "partitions=8")
    eng.close()
    # off the default launch geometry: the kernel always launches 512 threads over the engine's grid and partition table
    for kw in (dict(threads_per_wg=256, waves_per_cu=4), dict(threads_per_wg=64, waves_per_cu=4), dict(waves_per_cu=1)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, **kw)
        _check_engine(pkg, eng, m, xs, f"geometry {kw}")
        eng.close()


def test_long_partitions(pkg):
    """8 partitions of several hundred packets each (the shape of test_gpu_long_partitions.py): a wave walks them all, every
    vector's carry with it."""
    m = signed(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41)
    packed = pkg.Packed(m, k=16, n_wave_partitions=8)
    assert packed.info()["packets_per_partition"] >= 300
    eng = pkg.SpMV.from_packed(packed, k=16, device=0)
    assert eng.info()["n_wave_partitions"] == 8
    _check_engine(pkg, eng, m, _xs(3, 1024, 42), "8 long partitions", packed)
    eng.close()


def test_rules_on_the_device(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 13), 13)
    has = np.zeros(m.rows, dtype=bool)
    has[m.row] = True
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    xs = _xs(20, 1024, 14)
    labels, best = _check_engine(pkg, eng, m, xs, "rules")
    # a duplicated vector never wins under its larger index: inside one pass (5 = 2) and across two passes (18 = 2)
    for dup_at in (5, 18):
        dup = xs.copy()
        dup[dup_at] = dup[2]
        l2, _ = _check_engine(pkg, eng, m, dup, f"duplicate at {dup_at}")
        assert not np.any(l2 == dup_at) and np.any(l2 == 2)
    # all-zero vectors: every row label 0 with +0.0f, in one pass and in two
    for count in (3, 20):
        l0, b0 = eng.assign(np.zeros((count, 1024), dtype=np.float32))
        assert np.all(l0 == 0) and np.all(bits(b0) == 0), count
    eng.close()
    # strictly negative vectors on a positive matrix: every non-empty row's best is negative (a running best that starts at 0 fails)
    pos = coo(pkg, m.rows, m.cols, m.row, m.col, np.abs(m.val) + np.float32(0.01))
    eng = pkg.SpMV(pos.row, pos.col, pos.val, pos.rows, pos.cols, k=8, device=0)
    neg = -(np.abs(_xs(20, 1024, 15)) + np.float32(0.01))
    for count in (4, 20):
        ln, bn = _check_engine(pkg, eng, pos, neg[:count], f"negative vectors count={count}")
        assert np.all(bn[has] < 0) and np.all(ln[~has] == 0) and np.all(bits(bn[~has]) == 0)
    eng.close()


def test_identity_with_the_scoring_path(pkg):
    """best[r] is what score_rows reports for row r and the winning vector, on the same engine."""
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 17), 17)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, first_row=500)
    xs = _xs(20, 1024, 18)
    labels, best = eng.assign(xs)
    ids = np.random.default_rng(3).choice(m.rows, 200, replace=False).astype(np.uint32)
    got = np.array([eng.score_rows(ids[i:i + 1] + np.uint32(500), xs[labels[ids[i]]])[0, 0] for i in range(ids.size)], dtype=np.float32)
    assert np.array_equal(bits(got), bits(best[ids]))
    # ... and no other vector scores strictly higher, nor an earlier one as high
    all_scores = eng.score_rows(ids + np.uint32(500), xs)  # [20, 200]
    want_l, want_b = pkg.nearest(all_scores)
    assert np.array_equal(want_l, labels[ids]) and np.array_equal(bits(want_b), bits(best[ids]))
    eng.close()


def test_enqueue_into_guarded_buffers(pkg):
    """Exactly rows labels and rows scores change: guard zones of 64 words on both sides of both outputs keep their sentinel; on the
    engine's stream and on a caller's stream; and dev_best = 0 with one pass gives the same labels."""
    import torch
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 31), 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, first_row=77)
    xs = _xs(33, 1024, 32)
    d_xs = torch.from_numpy(xs).cuda()
    packed = _packed_like(pkg, eng, m)
    side = torch.cuda.Stream()
    SENT = -7
    for count in (16, 33):
        want_l, want_b = packed.assign(xs[:count])
        for stream in (None, side):
            for with_best in (True, False):
                if not with_best and count > PASS[1024]:
                    continue
                lab = torch.empty(GUARD + m.rows + GUARD, dtype=torch.int32, device="cuda")
                bst = torch.empty(GUARD + m.rows + GUARD, dtype=torch.float32, device="cuda")
                bp = bst.data_ptr() + 4 * GUARD if with_best else 0
                if stream is None:
                    lab.fill_(SENT), bst.fill_(SENT)
                    torch.cuda.synchronize()  # torch's fills are complete before the engine's stream starts
                    eng.enqueue_assign(d_xs.data_ptr(), count, lab.data_ptr() + 4 * GUARD, bp)
                    eng.synchronize()
                else:
                    with torch.cuda.stream(side):
                        lab.fill_(SENT), bst.fill_(SENT)  # the fills run on the caller's stream, in front of the passes
                    eng.enqueue_assign(d_xs.data_ptr(), count, lab.data_ptr() + 4 * GUARD, bp, stream=side.cuda_stream)
                    done = torch.cuda.Event()
                    done.record(side)
                    done.synchronize()
                hl, hb = lab.cpu().numpy(), bst.cpu().numpy()
                assert np.all(hl[:GUARD] == SENT) and np.all(hl[GUARD + m.rows:] == SENT), "labels written outside [0, rows)"
                assert np.all(hb[:GUARD] == SENT) and np.all(hb[GUARD + m.rows:] == SENT), "scores written outside [0, rows)"
                assert np.array_equal(hl[GUARD:GUARD + m.rows].view(np.uint32), want_l), (count, stream is not None, with_best)
                if with_best:
                    assert np.array_equal(bits(hb[GUARD:GUARD + m.rows]), bits(want_b)), (count, stream is not None)
                else:
                    assert np.all(hb == SENT), "dev_best = 0, yet scores were written"
    eng.close()


def test_engine_state_is_untouched(pkg):
    import torch
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    d_q = torch.from_numpy(xq).cuda()
    d_xs = torch.from_numpy(_xs(20, 1024, 22)).cuda()
    d_lab = torch.zeros(m.rows, dtype=torch.int32, device="cuda")
    d_best = torch.zeros(m.rows, dtype=torch.float32, device="cuda")
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
    eng.enqueue_assign(d_xs.data_ptr(), 20, d_lab.data_ptr(), d_best.data_ptr())
    eng.enqueue_assign(d_xs.data_ptr(), 5, d_lab.data_ptr())
    eng.synchronize()
    res1, counters1 = eng.read_result(), eng.debug_counters()
    assert counters1 == counters0, "enqueue_assign moved a counter"
    assert np.array_equal(res0[1], res1[1]) and np.array_equal(bits(res0[0]), bits(res1[0])), "enqueue_assign changed the result pair"
    # a batch call right behind an unwaited assignment returns the same lists
    d_idx[1].zero_(), d_val[1].zero_()
    torch.cuda.synchronize()
    eng.enqueue_assign(d_xs.data_ptr(), 20, d_lab.data_ptr(), d_best.data_ptr())
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[1].data_ptr(), d_val[1].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_idx[1].cpu().numpy(), want_idx) and np.array_equal(bits(d_val[1].cpu().numpy()), want_val)
    eng.close()


def test_status_codes(pkg):
    import torch
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    SENT = -7
    d_lab = torch.full((m.rows,), SENT, dtype=torch.int32, device="cuda")
    d_best = torch.full((m.rows,), SENT, dtype=torch.float32, device="cuda")
    xs = _xs(17, 512, 62)
    d_xs = torch.from_numpy(xs).cuda()
    torch.cuda.synchronize()
    INVALID, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED
    lib, X, Lb, B = pkg._lib.lib(), d_xs.data_ptr(), d_lab.data_ptr(), d_best.data_ptr()
    h_lab = np.full(m.rows, SENT, dtype=np.int32)
    h_best = np.full(m.rows, SENT, dtype=np.float32)
    HX, HL, HB = xs.ctypes.data_as(C.POINTER(C.c_float)), h_lab.ctypes.data_as(C.POINTER(C.c_uint32)), h_best.ctypes.data_as(C.POINTER(C.c_float))

    def status_of(fn):
        try:
            fn()
        except pkg.TkspmvError as e:
            return e.status
        return 0

    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=prec)
        assert status_of(lambda: eng.enqueue_assign(X, 2, Lb, B)) == UNSUPPORTED, prec
        assert status_of(lambda: eng.assign(xs)) == UNSUPPORTED, prec
        assert lib.tkspmv_assign(eng._h, HX, 2, HL, HB) == UNSUPPORTED, prec
        assert status_of(lambda: eng.enqueue_assign(X, 0, Lb, B)) == INVALID, prec  # INVALID comes before UNSUPPORTED
        assert status_of(lambda: eng.enqueue_assign(X, 2, 0, B)) == INVALID, prec
        assert status_of(lambda: eng.enqueue_assign(0, 2, Lb, B)) == INVALID, prec
        eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    for count in (0, -1):
        assert status_of(lambda: eng.enqueue_assign(X, count, Lb, B)) == INVALID, count
        assert lib.tkspmv_assign(eng._h, HX, count, HL, HB) == INVALID, count
    assert status_of(lambda: eng.enqueue_assign(0, 2, Lb, B)) == INVALID
    assert status_of(lambda: eng.enqueue_assign(X, 2, 0, B)) == INVALID
    assert lib.tkspmv_assign(eng._h, None, 2, HL, HB) == INVALID and lib.tkspmv_assign(eng._h, HX, 2, None, HB) == INVALID
    assert status_of(lambda: eng.enqueue_assign(X, 17, Lb, 0)) == INVALID  # dev_best = 0 takes one pass: at most 16 vectors here
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(h_lab == SENT) and np.all(h_best == SENT), "a rejected call wrote its host output"
    assert np.all(d_lab.cpu().numpy() == SENT) and np.all(d_best.cpu().numpy() == SENT), "a rejected call wrote its device output"
    # what is allowed works: 16 vectors without dev_best, the host form without host_best at any count
    want_l, want_b = _packed_like(pkg, eng, m).assign(xs)
    eng.enqueue_assign(X, 16, Lb, 0)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_lab.cpu().numpy().view(np.uint32), _packed_like(pkg, eng, m).assign(xs[:16])[0]) and np.all(d_best.cpu().numpy() == SENT)
    assert lib.tkspmv_assign(eng._h, HX, 17, HL, None) == 0
    assert np.array_equal(h_lab.view(np.uint32), want_l) and np.all(h_best == SENT)
    with pytest.raises(ValueError):
        eng.assign(xs[:, :-1])
    eng.close()


def test_installing_the_labels(pkg):
    """assign(install=True): the labels become the group labels, and run_grouped returns each cluster once, by its best row."""
    m = signed(pkg, pkg.generate_matrix(5000, 1024, 20, "gamma", 71), 71)
    count, k = 12, 16
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, min_score=-np.inf)
    labels, _ = eng.assign(_xs(count, 1024, 72), install=True)
    assert len(set(labels.tolist())) == count
    x = _xs(1, 1024, 73)[0]
    val, idx, grp = eng.run_grouped(vec=x)
    assert sorted(grp.tolist()) == list(range(count)), grp  # each cluster once (k >= count)
    has = np.zeros(m.rows, dtype=bool)
    has[m.row] = True
    y = eng.score_rows(np.arange(m.rows, dtype=np.uint32), x)[0]
    for v, i, g in zip(val, idx, grp):
        mine = has & (labels == g)
        assert labels[i] == g and bits(np.float32(v)) == bits(y[i]) and v == y[mine].max(), (g, i, v)
    lab2, best2 = pkg.assign_spmv(m, _xs(count, 1024, 72), device=0)  # the one-shot helper
    assert np.array_equal(lab2, labels)
    eng.close()
