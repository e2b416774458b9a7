"""Row statistics (tkspmv_enqueue_row_stats / tkspmv_row_stats / tkspmv_set_boost_cosine; SpMV.row_stats, set_cosine, cosine_spmv) on
the MI355X.

Everything is compared bit for bit. The expectation is the host twin, Packed.row_stats of a Packed built with the engine's own
geometry -- which test_row_stats_host.py pins to the order-matched oracle over the whole stream --, so the values are signed and
general here. On top: identities with the scoring paths of one engine (score_rows with the row's own vector as the query), the
cosine boost against the same weights installed through set_boost on a second engine, and the engine state a pass must not touch.
The conftest syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import bits, coo, signed
from test_score_rows_host import _hand_made

pytestmark = pytest.mark.gpu

FILL, GUARD = -7.0, 64
KINDS = (0, 1, 2, 3)


def _twin(pkg, eng, m, packed=None):
    """The host twin's four arrays for the engine's own layout (the geometry as test_gpu_score_rows.py takes it)."""
    info = eng.info()
    if packed is None:
        packed = pkg.Packed(m, k=eng.k, nnz_per_lane=info["packet_entries"] // 64, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    return [packed.row_stats(kind) for kind in KINDS]


def _check_engine(pkg, eng, m, label, packed=None):
    want = _twin(pkg, eng, m, packed)
    for kind in KINDS:
        got = eng.row_stats(kind)
        assert got.shape == (m.rows,) and got.dtype == np.float32
        bad = np.flatnonzero(bits(got) != bits(want[kind]))
        assert bad.size == 0, f"{label} kind {kind}: {bad.size} rows differ from the host twin, first {bad[:8]}: {got[bad[:8]]} != {want[kind][bad[:8]]}"
    assert np.array_equal(want[0], np.bincount(m.row, minlength=m.rows).astype(np.float32)), label
    return want


GENERATED = [(cols, c_lane) for cols in (300, 1024, 4096) for c_lane in (4, 8) if not (c_lane == 8 and cols > 1024)]


@pytest.mark.parametrize("cols,c_lane", GENERATED + [(4096, 8)])
def test_generated_matrices(pkg, cols, c_lane):
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, "gamma" if cols == 1024 else "uniform", 5 + cols), cols)
    if c_lane == 8 and cols > 1024:  # (8 entries per lane exist up to 1024 columns: creation refuses, nothing to compare)
        with pytest.raises(pkg.TkspmvError):
            pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, nnz_per_lane=c_lane).close()
        return
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, nnz_per_lane=c_lane)
    assert eng.info()["packet_entries"] == 64 * c_lane
    _check_engine(pkg, eng, m, f"2500x{cols} C={c_lane}")
    eng.close()


def _hand_made_general(pkg):
    """The 15-row matrix of test_score_rows_host.py (signed normal values; empty rows 0, 1, 4, 9 and 12..14; rows of 256, 512 and 1500
    entries) with a row of values near 1e-20 (12: its L2SQ is subnormal) and one near 1e25 (13: its L2SQ is +inf)."""
    base, _ = _hand_made(pkg, 1024)
    rng = np.random.default_rng(5)
    row = np.concatenate([base.row, np.full(8, 12), np.full(8, 13)])
    col = np.concatenate([base.col, rng.integers(0, 1024, 16)])
    val = np.concatenate([base.val, (1.0 + rng.random(8)) * 1e-20 * np.array([1, -1] * 4), (1.0 + rng.random(8)) * 1e25 * np.array([-1, 1] * 4)])
    return coo(pkg, base.rows, 1024, row, col, val)


@pytest.mark.parametrize("c_lane", [4, 8])
def test_hand_made_rows(pkg, c_lane):
    m = _hand_made_general(pkg)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
    nnz, l1, l2sq, inv = _check_engine(pkg, eng, m, f"hand-made C={c_lane}")
    for a in (nnz, l1, l2sq, inv):
        assert np.all(bits(a[[0, 1, 4, 9, 14]]) == 0)
    assert nnz[3] == 256 and nnz[5] == 512 and nnz[6] == 1500
    assert 0 < l2sq[12] < np.finfo(np.float32).tiny and np.isfinite(inv[12]) and inv[12] > 1e19
    assert np.isposinf(l2sq[13]) and bits(inv[13:14])[0] == 0
    assert np.array_equal(bits(inv), bits(pkg.inv_l2(l2sq))) and np.all(np.isfinite(eng.row_stats(pkg._lib.ROW_INV_L2)))
    eng.close()


def test_partition_tails(pkg):
    rng = np.random.default_rng(7)
    rows, per = 128, 8  # 1024 entries: rows end on the last slot of a packet
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    for c_lane in (4, 8):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
        _check_engine(pkg, eng, m, f"exact fit C={c_lane}")
        eng.close()


def test_from_packed_first_row_approximate_and_geometry(pkg, tmp_path):
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 9), 9)
    # an engine made from a saved and loaded file: no COO anywhere near it
    hint = pkg.Packed.wave_partitions(device=0, m=m)
    packed = pkg.Packed(m, k=16, n_wave_partitions=hint)
    packed.save(tmp_path / "m.tkspmv")
    eng = pkg.SpMV.from_packed(pkg.Packed.load(tmp_path / "m.tkspmv"), k=16, device=0)
    _check_engine(pkg, eng, m, "from_packed", packed)
    eng.close()
    # first_row: the outputs are indexed by LOCAL row
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, first_row=1000)
    _check_engine(pkg, eng, m, "first_row=1000")
    eng.close()
    # an approximate per-partition engine is served
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    _check_engine(pkg, eng, m, "partitions=8")
    eng.close()
    # off the default launch geometry: the kernel always launches 512 threads over the engine's grid and partition table
    for kw in (dict(threads_per_wg=256, waves_per_cu=4), dict(threads_per_wg=64, waves_per_cu=4), dict(waves_per_cu=1)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, **kw)
        _check_engine(pkg, eng, m, f"geometry {kw}")
        eng.close()


def test_long_partitions(pkg):
    """8 partitions of several hundred packets each (the shape of test_gpu_long_partitions.py): a wave walks them all."""
    m = signed(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41)
    packed = pkg.Packed(m, k=16, n_wave_partitions=8)
    assert packed.info()["packets_per_partition"] >= 300
    eng = pkg.SpMV.from_packed(packed, k=16, device=0)
    assert eng.info()["n_wave_partitions"] == 8
    _check_engine(pkg, eng, m, "8 long partitions", packed)
    eng.close()


def test_enqueue_into_a_guarded_buffer(pkg):
    """Exactly rows floats change: guard zones of 64 floats on both sides keep their sentinel; on the engine's stream and on a
    caller's stream with the caller's event waited for."""
    import torch
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 31), 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, first_row=77)
    want = _twin(pkg, eng, m)
    side = torch.cuda.Stream()
    for stream in (None, side):
        for kind in KINDS:
            buf = torch.empty(GUARD + m.rows + GUARD, dtype=torch.float32, device="cuda")
            if stream is None:
                buf.fill_(FILL)
                torch.cuda.synchronize()  # torch's fill is complete before the engine's stream starts
                eng.enqueue_row_stats(kind, buf.data_ptr() + 4 * GUARD)
                eng.synchronize()
            else:
                with torch.cuda.stream(side):
                    buf.fill_(FILL)  # the fill runs on the caller's stream, in front of the pass
                eng.enqueue_row_stats(kind, buf.data_ptr() + 4 * GUARD, stream=side.cuda_stream)
                done = torch.cuda.Event()
                done.record(side)
                done.synchronize()
            out = buf.cpu().numpy()
            assert np.all(bits(out[:GUARD]) == bits(np.float32(FILL))) and np.all(bits(out[GUARD + m.rows:]) == bits(np.float32(FILL))), "written outside [0, rows)"
            assert np.array_equal(bits(out[GUARD:GUARD + m.rows]), bits(want[kind])), (stream is not None, kind)
    eng.close()


def test_identity_with_the_scoring_paths(pkg):
    """L2SQ of row r == score_rows([r], vecs=row_vectors([r])): the row scored against itself, on matrices without repeated columns."""
    L = pkg._lib
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 17), 17)
    key = m.row.astype(np.uint64) * np.uint64(1 << 20) + m.col.astype(np.uint64)
    keep = np.unique(key, return_index=True)[1]  # (the first entry of every (row, column))
    m = coo(pkg, m.rows, m.cols, m.row[keep], m.col[keep], m.val[keep])
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    l2sq = eng.row_stats(L.ROW_L2SQ)
    ids = np.random.default_rng(3).choice(m.rows, 200, replace=False).astype(np.uint32)
    rv, _ = eng.row_vectors(ids)
    got = np.array([eng.score_rows(ids[i:i + 1], rv[i])[0, 0] for i in range(ids.size)], dtype=np.float32)
    assert np.array_equal(bits(got), bits(l2sq[ids]))
    assert np.count_nonzero(l2sq[ids]) >= 190
    eng.close()
    base, _ = _hand_made(pkg, 1024)
    key = base.row.astype(np.uint64) * np.uint64(1 << 20) + base.col.astype(np.uint64)
    keep = np.sort(np.unique(key, return_index=True)[1])
    m = coo(pkg, base.rows, 1024, base.row[keep], base.col[keep], base.val[keep])
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0)
    l2sq = eng.row_stats(L.ROW_L2SQ)
    ids = np.arange(m.rows, dtype=np.uint32)
    rv, _ = eng.row_vectors(ids)
    got = np.array([eng.score_rows(ids[i:i + 1], rv[i])[0, 0] for i in range(ids.size)], dtype=np.float32)
    assert np.array_equal(bits(got), bits(l2sq))
    eng.close()


def _unit(x):
    v = np.asarray(x, dtype=np.float64)
    return (v / np.sqrt(np.sum(v * v))).astype(np.float32)


def test_cosine_boost(pkg, tmp_path):
    L = pkg._lib
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 23), 23)
    k = 20
    x = _unit(np.random.default_rng(4).standard_normal(m.cols))
    a = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, vec=x, min_score=-np.inf)
    b = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, vec=x, min_score=-np.inf)
    weight = pkg.inv_l2(_twin(pkg, b, m)[L.ROW_L2SQ])
    allow = np.random.default_rng(5).random(m.rows) < 0.3

    def pages(eng, n_pages, allow=None, **boost):
        out, cursor = [], None
        for _ in range(n_pages):
            idx, val, n, total, cursor = eng.run_boosted(cursor, allow=allow, **boost)
            out.append((idx.copy(), bits(val).copy(), n, total, tuple(cursor)))
            boost = {}
        return out

    def same(p, q):
        return len(p) == len(q) and all(np.array_equal(s[0], t[0]) and np.array_equal(s[1], t[1]) and s[2:] == t[2:] for s, t in zip(p, q))

    # a bias installed before set_cosine() is removed by it
    a.set_boost(bias=np.full(m.rows, 5.0, np.float32))
    a.set_cosine()
    assert same(pages(a, 1), pages(b, 1, weight=weight)), "set_cosine() differs from set_boost(weight=inv_l2(L2SQ))"
    assert same(pages(a, 3), pages(b, 3)), "three chained pages differ"
    assert same(pages(a, 3, allow=allow), pages(b, 3, allow=allow)), "three chained pages under an allow-mask differ"
    idx, val, n, _, _ = a.run_boosted()
    assert n == k and np.all(val[:n] <= 1 + 1e-6) and np.all(val[:n] >= -1 - 1e-6)
    a.close()
    b.close()
    # an engine from a .tkspmv file gets cosine without the COO matrix
    packed = pkg.Packed(m, k=k, n_wave_partitions=pkg.Packed.wave_partitions(device=0, m=m))
    packed.save(tmp_path / "m.tkspmv")
    loaded = pkg.Packed.load(tmp_path / "m.tkspmv")
    c = pkg.SpMV.from_packed(loaded, k=k, device=0, vec=x, min_score=-np.inf)
    d = pkg.SpMV.from_packed(loaded, k=k, device=0, vec=x, min_score=-np.inf)
    c.set_cosine()
    assert same(pages(c, 2), pages(d, 2, weight=pkg.inv_l2(loaded.row_stats(L.ROW_L2SQ))))
    c.close()
    d.close()


def test_cosine_spmv(pkg):
    m = signed(pkg, pkg.generate_matrix(5000, 1024, 20, "gamma", 29), 29)
    q = np.zeros(m.cols, dtype=np.float32)
    np.add.at(q, m.col[m.row == 7], m.val[m.row == 7])
    assert np.count_nonzero(m.row == 7) >= 2
    val, idx = pkg.cosine_spmv(m, 3.0 * q, 10, device=0)  # (any positive multiple of row 7: the helper scales it to norm 1)
    assert idx[0] == 7 and abs(float(val[0]) - 1.0) <= 4 * 2.0 ** -24, (idx[:3], val[:3])
    assert np.all(val <= 1 + 1e-6) and np.all(val >= -1 - 1e-6) and np.all(np.diff(val) <= 0)
    allow = np.ones(m.rows, dtype=bool)
    allow[7] = False
    val2, idx2 = pkg.cosine_spmv(m, q, 10, allow=allow, device=0)
    assert 7 not in idx2 and np.all(val2 <= 1 + 1e-6) and np.all(val2 >= -1 - 1e-6)
    val0, idx0 = pkg.cosine_spmv(m, np.zeros(m.cols, np.float32), 10, device=0)  # a zero vector stays zero
    assert np.all(val0 == 0)


def test_engine_state_is_untouched(pkg):
    import torch
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    d_q = torch.from_numpy(xq).cuda()
    d_out = torch.zeros(m.rows, dtype=torch.float32, device="cuda")
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
    for kind in KINDS:
        eng.enqueue_row_stats(kind, d_out.data_ptr())
    eng.synchronize()
    res1, counters1 = eng.read_result(), eng.debug_counters()
    assert counters1 == counters0, "enqueue_row_stats moved a counter"
    assert np.array_equal(res0[1], res1[1]) and np.array_equal(bits(res0[0]), bits(res1[0])), "enqueue_row_stats changed the result pair"
    # a batch call right behind an unwaited pass returns the same lists
    d_idx[1].zero_(), d_val[1].zero_()
    torch.cuda.synchronize()
    eng.enqueue_row_stats(2, d_out.data_ptr())
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[1].data_ptr(), d_val[1].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_idx[1].cpu().numpy(), want_idx) and np.array_equal(bits(d_val[1].cpu().numpy()), want_val)
    eng.close()


def test_status_codes(pkg):
    import torch
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    d_out = torch.full((m.rows,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    INVALID, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED
    lib, O = pkg._lib.lib(), d_out.data_ptr()
    h_out = np.full(m.rows, FILL, dtype=np.float32)

    def status_of(fn):
        try:
            fn()
        except pkg.TkspmvError as e:
            return e.status
        return 0

    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=prec)
        assert status_of(lambda: eng.enqueue_row_stats(2, O)) == UNSUPPORTED, prec
        assert status_of(lambda: eng.row_stats(2)) == UNSUPPORTED, prec
        assert status_of(lambda: eng.set_cosine()) == UNSUPPORTED, prec
        assert status_of(lambda: eng.enqueue_row_stats(4, O)) == INVALID, prec  # INVALID comes before UNSUPPORTED
        assert status_of(lambda: eng.enqueue_row_stats(2, 0)) == INVALID, prec
        eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    for kind in (-1, 4):
        assert status_of(lambda: eng.enqueue_row_stats(kind, O)) == INVALID, kind
        assert lib.tkspmv_row_stats(eng._h, kind, h_out.ctypes.data_as(C.POINTER(C.c_float))) == INVALID, kind
    assert status_of(lambda: eng.enqueue_row_stats(0, 0)) == INVALID
    assert lib.tkspmv_row_stats(eng._h, 0, None) == INVALID
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(h_out == FILL) and np.all(bits(d_out.cpu().numpy()) == bits(np.float32(FILL))), "a rejected call wrote its output"
    eng.enqueue_row_stats(0, O)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), np.bincount(m.row, minlength=m.rows).astype(np.float32))
    eng.close()
