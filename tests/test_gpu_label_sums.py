"""Label sums (tkspmv_enqueue_label_sums / _sums_close / _sums_exponent / tkspmv_label_sums; SpMV.enqueue_label_sums,
enqueue_sums_close, sums_exponent, label_sums, kmeans) on the MI355X.

The sums are integers: everything is compared exactly, int64 against int64 and float bits against float bits. The expectation is the
host twin Packed.label_sums -- which test_label_sums_host.py pins to the contract from the COO --, and, the sums being independent
of every layout, host.label_sums from the COO itself. Both sinks of the kernel are forced on every shape (the LDS sink exists up to
4096 columns), with bin counts on both sides of what one launch of the LDS sink holds (8 / 2 bins at 1024 / 4096 columns). Every
device output lies between guard zones. The conftest syncs torch only for the older enqueue names: these tests synchronise themselves."""
import ctypes as C

import numpy as np
import pytest

from support import GuardedOut, bits, coo, signed, status_of
from test_label_sums_host import _labels, _wide
from test_score_rows_host import _hand_made

pytestmark = pytest.mark.gpu


class SumsOut(GuardedOut):
    """One call's int64 sums (two 32-bit words each: the guard zones are counted in words) and float output."""
    def __init__(self, torch, n_bins, cols):
        self.COLUMNS = (("dev_sums", 2 * n_bins * cols, "int32"), ("dev_out", n_bins * cols, "float32"))
        super().__init__(torch, 1, 0)
        self.shape = (n_bins, cols)

    def read(self):
        res = super().read()
        return res["dev_sums"].reshape(-1).view(np.int64).reshape(self.shape).copy(), res["dev_out"].reshape(self.shape).copy()


def _packed_like(pkg, eng, m):
    info = eng.info()
    packed = pkg.Packed(m, k=eng.k, nnz_per_lane=info["packet_entries"] // 64, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    return packed


def _sinks(pkg, cols):
    L = pkg._lib
    return ((L.SUMS_SINK_LDS, "lds"), (L.SUMS_SINK_DIRECT, "direct"), (0, "auto")) if cols <= 4096 else ((L.SUMS_SINK_DIRECT, "direct"), (0, "auto"))


def _enqueue(pkg, torch, eng, lab, n_bins, e, mode, flags=0, prev=None, stream=None):
    """One enqueue_label_sums into guarded buffers: (sums int64[n_bins, cols], out float32[n_bins, cols]); out starts as prev (-7
    without one, which is also what RAW must leave)."""
    out = SumsOut(torch, n_bins, eng.num_cols)
    if prev is not None:
        out.dev["dev_out"][64:64 + prev.size] = torch.from_numpy(np.ascontiguousarray(prev, dtype=np.float32).ravel()).cuda()
    d_lab = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    p = out.ptrs()
    eng.enqueue_label_sums(d_lab.data_ptr(), n_bins, e, p["dev_sums"], mode, p["dev_out"] if mode != pkg._lib.SUMS_RAW else 0, flags, stream=stream or 0)
    eng.synchronize()
    torch.cuda.synchronize()
    return out.read()


def _check_engine(pkg, torch, eng, m, bins, label, packed=None, exps=None):
    """Every sink, bin count, exponent and mode: int64 sums == the twin's == the contract's from the COO; floats == the twin's bits."""
    packed = _packed_like(pkg, eng, m) if packed is None else packed
    RAW, FLOAT, UNIT = pkg._lib.SUMS_RAW, pkg._lib.SUMS_FLOAT, pkg._lib.SUMS_UNIT
    default = eng.sums_exponent()
    assert default == packed.sums_exponent() == pkg.sums_exponent(m), label
    for n_bins in bins:
        lab = _labels(m.rows, n_bins, n_bins)
        prev = np.random.default_rng(n_bins).standard_normal((n_bins, m.cols)).astype(np.float32)
        for e in exps or (default, -12):
            want = pkg.label_sums(m, lab, n_bins, e)
            twin_sums, twin_f = packed.label_sums(lab, n_bins, e, FLOAT)
            _, twin_u = packed.label_sums(lab, n_bins, e, UNIT, out=prev)
            assert np.array_equal(twin_sums, want), label
            for flags, sink in _sinks(pkg, m.cols):
                where = f"{label} n_bins={n_bins} E={e} sink={sink}"
                for mode, expect in ((RAW, None), (FLOAT, twin_f), (UNIT, twin_u)):
                    sums, out = _enqueue(pkg, torch, eng, lab, n_bins, e, mode, flags, prev if mode == UNIT else None)
                    bad = np.argwhere(sums != want)
                    assert bad.size == 0, f"{where} mode={mode}: {len(bad)} words differ, first {bad[:4].tolist()}: {sums[tuple(bad[0])]} != {want[tuple(bad[0])]}"
                    if expect is None:
                        assert np.all(out == -7), f"{where}: RAW wrote dev_out"
                    else:
                        assert np.array_equal(bits(out), bits(expect)), f"{where} mode={mode}: float bits differ from the twin"
    return default


GENERATED = [(2500, 300, 4, (1, 2, 8, 9, 17)), (2500, 1024, 4, (1, 2, 8, 9, 17)), (2500, 1024, 8, (1, 2, 8, 9, 17)), (2500, 4096, 4, (1, 2, 3, 5)),
             (600, 5000, 4, (1, 3))]


@pytest.mark.parametrize("rows,cols,c_lane,bins", GENERATED)
def test_generated_matrices(pkg, rows, cols, c_lane, bins):
    import torch
    m = _wide(pkg, pkg.generate_matrix(rows, cols, 20, "gamma" if cols == 1024 else "uniform", 7 + cols), cols)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, nnz_per_lane=c_lane)
    assert eng.info()["packet_entries"] == 64 * c_lane
    _check_engine(pkg, torch, eng, m, bins, f"{rows}x{cols} C={c_lane}")
    eng.close()


@pytest.mark.parametrize("c_lane", [4, 8])
def test_hand_made_rows(pkg, c_lane):
    """Empty rows in front, in the middle and at the end; rows of 256, 512 and 1500 entries, which cross packets and keep their label."""
    import torch
    m, _ = _hand_made(pkg, 1024)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
    _check_engine(pkg, torch, eng, m, (1, 3, 9), f"hand-made C={c_lane}", exps=(eng.sums_exponent(), -8))
    eng.close()


def test_partition_tails_and_padding(pkg):
    import torch
    rng = np.random.default_rng(7)
    rows, per = 128, 8  # 1024 entries: rows end on the last slot of a packet
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    # no entry in column 0 and a stream that ends in padding: column 0 stays 0 (host test: test_padding_never_reaches_column_0)
    col = np.stack([rng.choice(np.arange(1, 64), 7, replace=False) for _ in range(300)]).ravel()
    p = coo(pkg, 300, 64, np.repeat(np.arange(300), 7), col, rng.standard_normal(300 * 7) + 3.0)
    for c_lane in (4, 8):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
        _check_engine(pkg, torch, eng, m, (1, 9), f"exact fit C={c_lane}")
        eng.close()
        eng = pkg.SpMV(p.row, p.col, p.val, p.rows, p.cols, k=4, device=0, nnz_per_lane=c_lane)
        _check_engine(pkg, torch, eng, p, (1, 3), f"padding C={c_lane}", exps=(-20,))
        for flags, sink in _sinks(pkg, 64):
            sums, _ = _enqueue(pkg, torch, eng, np.zeros(300, dtype=np.uint32), 1, -20, pkg._lib.SUMS_RAW, flags)
            assert sums[0, 0] == 0 and np.all(sums[0, 1:] > 0), sink
        eng.close()


def test_from_packed_first_row_approximate_and_geometry(pkg, tmp_path):
    """An engine from a loaded file, first_row, an approximate engine, three launch geometries and 8 long partitions: all give the
    sums the COO gives -- the claim that the geometry does not matter."""
    import torch
    m = _wide(pkg, pkg.generate_matrix(6000, 1024, 20, "gamma", 9), 9)
    n_bins, e = 9, pkg.sums_exponent(m)
    lab = _labels(m.rows, n_bins, 4)
    want = pkg.label_sums(m, lab, n_bins, e)
    hint = pkg.Packed.wave_partitions(device=0, m=m)
    packed = pkg.Packed(m, k=16, n_wave_partitions=hint)
    packed.save(tmp_path / "m.tkspmv")
    long8 = pkg.Packed(_wide(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41), k=16, n_wave_partitions=8)
    assert long8.info()["packets_per_partition"] >= 300
    engines = [("from_packed", lambda: pkg.SpMV.from_packed(pkg.Packed.load(tmp_path / "m.tkspmv"), k=16, device=0)),
               ("first_row=1000", lambda: pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, first_row=1000)),
               ("partitions=8", lambda: pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0))]
    for kw in (dict(threads_per_wg=256, waves_per_cu=4), dict(threads_per_wg=64, waves_per_cu=4), dict(waves_per_cu=1)):
        engines.append((f"geometry {kw}", lambda kw=kw: pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, **kw)))
    for name, make in engines:
        eng = make()
        assert eng.sums_exponent() == e, name
        for flags, sink in _sinks(pkg, 1024):
            sums, _ = _enqueue(pkg, torch, eng, lab, n_bins, e, pkg._lib.SUMS_RAW, flags)
            assert np.array_equal(sums, want), (name, sink)
        eng.close()
    m8 = _wide(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41)
    eng = pkg.SpMV.from_packed(long8, k=16, device=0)
    assert eng.info()["n_wave_partitions"] == 8
    lab8, e8 = _labels(m8.rows, n_bins, 5), pkg.sums_exponent(m8)
    want8 = pkg.label_sums(m8, lab8, n_bins, e8)
    for flags, sink in _sinks(pkg, 1024):
        sums, _ = _enqueue(pkg, torch, eng, lab8, n_bins, e8, pkg._lib.SUMS_RAW, flags)
        assert np.array_equal(sums, want8), ("8 long partitions", sink)
    eng.close()


def test_accumulate_merges_the_halves_of_a_matrix(pkg):
    """Two engines over the row halves, one common exponent (the larger of theirs), one buffer: the sums of the whole matrix; then
    enqueue_sums_close gives the whole's FLOAT and UNIT bits."""
    import torch
    L = pkg._lib
    m = _wide(pkg, pkg.generate_matrix(5000, 1024, 20, "gamma", 51), 51)
    cut = 2311
    top, bot = m.row < cut, m.row >= cut
    halves = [coo(pkg, cut, m.cols, m.row[top], m.col[top], m.val[top]), coo(pkg, m.rows - cut, m.cols, m.row[bot] - cut, m.col[bot], m.val[bot])]
    n_bins = 9
    lab = _labels(m.rows, n_bins, 6)
    engs = [pkg.SpMV(h.row, h.col, h.val, h.rows, h.cols, k=8, device=0, first_row=f) for h, f in zip(halves, (0, cut))]
    whole = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    e = max(x.sums_exponent() for x in engs)
    assert e <= whole.sums_exponent()
    want = pkg.label_sums(m, lab, n_bins, e)
    prev = np.full((n_bins, m.cols), 2.5, dtype=np.float32)
    w_sums, w_float = _enqueue(pkg, torch, whole, lab, n_bins, e, L.SUMS_FLOAT)
    _, w_unit = _enqueue(pkg, torch, whole, lab, n_bins, e, L.SUMS_UNIT, prev=prev)
    assert np.array_equal(w_sums, want)
    for flags, sink in _sinks(pkg, 1024):
        out = SumsOut(torch, n_bins, m.cols)
        d_labs = [torch.from_numpy(part.view(np.int32).copy()).cuda() for part in (lab[:cut], lab[cut:])]
        torch.cuda.synchronize()
        p = out.ptrs()
        engs[0].enqueue_label_sums(d_labs[0].data_ptr(), n_bins, e, p["dev_sums"], L.SUMS_RAW, 0, flags)  # zeroes the buffer in front
        engs[0].synchronize()
        engs[1].enqueue_label_sums(d_labs[1].data_ptr(), n_bins, e, p["dev_sums"], L.SUMS_RAW, 0, flags | L.SUMS_ACCUMULATE)
        engs[1].synchronize()
        sums, untouched = out.read()
        assert np.array_equal(sums, want) and np.all(untouched == -7), sink
        engs[1].enqueue_sums_close(p["dev_sums"], n_bins, e, L.SUMS_FLOAT, p["dev_out"])
        engs[1].synchronize()
        assert np.array_equal(bits(out.read()[1]), bits(w_float)), sink
        out.dev["dev_out"][64:64 + prev.size] = torch.from_numpy(prev.ravel()).cuda()
        torch.cuda.synchronize()
        engs[0].enqueue_sums_close(p["dev_sums"], n_bins, e, L.SUMS_UNIT, p["dev_out"])
        engs[0].synchronize()
        assert np.array_equal(bits(out.read()[1]), bits(w_unit)), sink
    for x in engs + [whole]:
        x.close()


def test_installed_labels_and_the_host_form(pkg):
    m = signed(pkg, pkg.generate_matrix(5000, 1024, 20, "gamma", 71), 71)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0)
    assert status_of(pkg, eng.label_sums) == pkg._lib.ERR_INVALID  # no labels installed
    xs = np.random.default_rng(72).standard_normal((12, 1024)).astype(np.float32)
    labels, _ = eng.assign(xs, install=True)
    e = eng.sums_exponent()
    want = pkg.label_sums(m, labels, 12, e)
    sums, none = eng.label_sums()  # dev_labels = NULL, n_bins = 0: the installed labels and their count
    assert none is None and np.array_equal(sums, want)
    sums, f = eng.label_sums(labels, 12, pkg._lib.SUMS_FLOAT, exp=e)
    assert np.array_equal(sums, want) and np.array_equal(bits(f), bits(pkg.close_sums(want, e, pkg._lib.SUMS_FLOAT)))
    prev = np.full((14, 1024), 4.0, dtype=np.float32)  # bins 12 and 13 are empty: they keep their rows
    sums, u = eng.label_sums(labels, 14, pkg._lib.SUMS_UNIT, exp=e, out=prev)
    assert np.array_equal(bits(u), bits(pkg.close_sums(pkg.label_sums(m, labels, 14, e), e, pkg._lib.SUMS_UNIT, out=prev))) and np.all(u[12:] == 4.0)
    eng.close()


def _twin_chain(pkg, packed, cent, e, iters):
    for _ in range(iters):
        labels, _ = packed.assign(cent)
        _, cent = packed.label_sums(labels, cent.shape[0], e, pkg._lib.SUMS_UNIT, out=cent)
    labels, best = packed.assign(cent)
    return cent, labels, best


def _start(count, cols, seed):
    """Positive unit vectors and, last, a negative one: on a positive matrix it scores below every other vector in every row, in
    every iteration -- its cluster ends empty each time and keeps its vector."""
    cent = np.abs(np.random.default_rng(seed).standard_normal((count, cols))).astype(np.float32)
    cent[count - 1] = -cent[1]
    return (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float32)


def _positive(pkg, m):
    return coo(pkg, m.rows, m.cols, m.row, m.col, np.abs(m.val) + np.float32(0.01))


def test_kmeans_chain_on_a_callers_stream(pkg):
    """enqueue_assign -> enqueue_label_sums(UNIT, dev_out = the vectors of the next assign), twice, on a caller's stream with no wait
    in between: centroids, labels and scores equal the twin chain's as bits; the negative centroid's cluster ends empty and keeps its
    vector."""
    import torch
    m = _positive(pkg, pkg.generate_matrix(5000, 1024, 20, "gamma", 81))
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    packed = _packed_like(pkg, eng, m)
    count, e = 9, eng.sums_exponent()
    cent0 = _start(count, 1024, 82)
    side = torch.cuda.Stream()
    for flags, sink in _sinks(pkg, 1024):
        d_xs = torch.from_numpy(cent0).cuda()
        d_lab = torch.zeros(m.rows, dtype=torch.int32, device="cuda")
        d_best = torch.zeros(m.rows, dtype=torch.float32, device="cuda")
        d_sums = torch.zeros(count * 1024, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            eng.enqueue_assign(d_xs.data_ptr(), count, d_lab.data_ptr(), d_best.data_ptr(), stream=side.cuda_stream)
            eng.enqueue_label_sums(d_lab.data_ptr(), count, e, d_sums.data_ptr(), pkg._lib.SUMS_UNIT, d_xs.data_ptr(), flags, stream=side.cuda_stream)
        eng.enqueue_assign(d_xs.data_ptr(), count, d_lab.data_ptr(), d_best.data_ptr(), stream=side.cuda_stream)
        done = torch.cuda.Event()
        done.record(side)
        done.synchronize()
        want_c, want_l, want_b = _twin_chain(pkg, packed, cent0, e, 2)
        got_c = d_xs.cpu().numpy()
        assert np.array_equal(bits(got_c), bits(want_c)), sink
        assert np.array_equal(d_lab.cpu().numpy().view(np.uint32), want_l) and np.array_equal(bits(d_best.cpu().numpy()), bits(want_b)), sink
        assert np.array_equal(bits(got_c[count - 1]), bits(cent0[count - 1])) and not np.any(want_l == count - 1), "the empty cluster keeps its vector"
        assert not np.array_equal(bits(got_c[0]), bits(cent0[0]))
    eng.close()


def test_kmeans_helpers(pkg):
    m = _positive(pkg, pkg.generate_matrix(3000, 300, 12, "gamma", 91))
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    cent0 = _start(6, 300, 92)
    want = _twin_chain(pkg, _packed_like(pkg, eng, m), cent0, eng.sums_exponent(), 3)
    got = eng.kmeans(cent0, 3)
    eng.close()
    one = pkg.kmeans_spmv(m, cent0, 3, device=0)
    for g in (got, one):
        assert np.array_equal(bits(g[0]), bits(want[0])) and np.array_equal(g[1], want[1]) and np.array_equal(bits(g[2]), bits(want[2]))


def test_engine_state_is_untouched(pkg):
    import torch
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    d_q = torch.from_numpy(xq).cuda()
    d_lab = torch.from_numpy(_labels(m.rows, 20, 3).view(np.int32)).cuda()
    d_sums = torch.zeros(20 * 1024, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(20 * 1024, dtype=torch.float32, device="cuda")
    d_idx = [torch.zeros((8, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    d_val = [torch.zeros((8, k), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    e = eng.sums_exponent()
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[0].data_ptr(), d_val[0].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    want_idx, want_val = d_idx[0].cpu().numpy().copy(), bits(d_val[0].cpu().numpy()).copy()
    eng.enqueue_batch(d_q.data_ptr(), 8)  # (engine-owned result pair: the last query wins)
    eng.synchronize()
    res0, counters0 = eng.read_result(), eng.debug_counters()
    for flags in (pkg._lib.SUMS_SINK_LDS, pkg._lib.SUMS_SINK_DIRECT):
        eng.enqueue_label_sums(d_lab.data_ptr(), 20, e, d_sums.data_ptr(), pkg._lib.SUMS_UNIT, d_out.data_ptr(), flags)
    eng.synchronize()
    res1, counters1 = eng.read_result(), eng.debug_counters()
    assert counters1 == counters0, "enqueue_label_sums moved a counter"
    assert np.array_equal(res0[1], res1[1]) and np.array_equal(bits(res0[0]), bits(res1[0])), "enqueue_label_sums changed the result pair"
    # a batch call right behind unwaited label sums returns the same lists
    eng.enqueue_label_sums(d_lab.data_ptr(), 20, e, d_sums.data_ptr(), pkg._lib.SUMS_FLOAT, d_out.data_ptr())
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[1].data_ptr(), d_val[1].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_idx[1].cpu().numpy(), want_idx) and np.array_equal(bits(d_val[1].cpu().numpy()), want_val)
    eng.close()


def test_status_codes(pkg):
    import torch
    L = pkg._lib
    INVALID, UNSUPPORTED = L.ERR_INVALID, L.ERR_UNSUPPORTED
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    wide = pkg.generate_matrix(600, 5000, 20, "uniform", 62)
    d_lab = torch.zeros(m.rows, dtype=torch.int32, device="cuda")
    d_sums = torch.full((2 * 512,), -7, dtype=torch.int64, device="cuda")
    d_out = torch.full((2 * 512,), -7, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    Lb, S, O = d_lab.data_ptr(), d_sums.data_ptr(), d_out.data_ptr()
    h_lab = np.zeros(m.rows, dtype=np.uint32)
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=prec)
        assert status_of(pkg, eng.enqueue_label_sums, Lb, 2, 0, S) == UNSUPPORTED, prec
        assert status_of(pkg, eng.sums_exponent) == UNSUPPORTED, prec
        assert status_of(pkg, eng.label_sums, h_lab, 2, exp=0) == UNSUPPORTED, prec
        assert status_of(pkg, eng.enqueue_label_sums, Lb, 2, 0, 0) == INVALID, prec  # INVALID comes before UNSUPPORTED
        assert status_of(pkg, eng.enqueue_label_sums, Lb, 2, 0, S, L.SUMS_FLOAT, 0) == INVALID, prec
        eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    bad = [(Lb, 2, 0, 0), (Lb, 2, 0, S + 4), (Lb, 0, 0, S), (0, 2, 0, S), (Lb, (1 << 30) + 1, 0, S), (Lb, 2, 0, S, 3, O), (Lb, 2, 0, S, -1, O),
           (Lb, 2, 0, S, L.SUMS_FLOAT, 0), (Lb, 2, 0, S, L.SUMS_UNIT, 0), (Lb, 2, 0, S, L.SUMS_RAW, 0, 8), (Lb, 2, 0, S, L.SUMS_RAW, 0, L.SUMS_SINK_LDS | L.SUMS_SINK_DIRECT),
           (0, 0, 0, S)]  # (the last: dev_labels = NULL with nothing installed)
    for args in bad:
        assert status_of(pkg, eng.enqueue_label_sums, *args) == INVALID, args
    for args in [(0, 2, 0, L.SUMS_FLOAT, O), (S, 2, 0, L.SUMS_FLOAT, 0), (S, 0, 0, L.SUMS_FLOAT, O), (S, 2, 0, L.SUMS_RAW, O), (S, 2, 0, 3, O), (S + 4, 2, 0, L.SUMS_UNIT, O)]:
        assert status_of(pkg, eng.enqueue_sums_close, *args) == INVALID, args
    assert pkg._lib.lib().tkspmv_sums_exponent(eng._h, None) == INVALID
    assert pkg._lib.lib().tkspmv_label_sums(eng._h, h_lab.ctypes.data_as(C.POINTER(C.c_uint32)), 2, 0, L.SUMS_FLOAT, None, None) == INVALID
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(d_sums.cpu().numpy() == -7) and np.all(d_out.cpu().numpy() == -7), "a rejected call wrote its output"
    eng.close()
    eng = pkg.SpMV(wide.row, wide.col, wide.val, wide.rows, wide.cols, k=8, device=0)  # the 16384-column tier has the direct sink only
    d_big = torch.full((5000,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert status_of(pkg, eng.enqueue_label_sums, Lb, 1, 0, d_big.data_ptr(), L.SUMS_RAW, 0, L.SUMS_SINK_LDS) == INVALID
    eng.synchronize()
    assert np.all(d_big.cpu().numpy() == -7)
    eng.close()
