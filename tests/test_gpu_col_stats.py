"""Column statistics (tkspmv_enqueue_col_stats / tkspmv_col_stats; SpMV.enqueue_col_stats, col_stats) on the MI355X.

Everything is compared exactly: words for COL_NNZ, bits for COL_MAX / COL_MIN. The expectation is host.col_stats on the COO and
Packed.col_stats -- the twin over the stream -- with the engine's own geometry; test_col_stats_host.py pins the two to each other.
The conftest syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import coo, signed
from test_col_stats_host import _u32, every_row_matrix, padding_leak_matrix
from test_gpu_match import _edges

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
SENTINEL, GUARD = 0xA5A5A5A5, 64


def _packed_twin(pkg, eng, m):
    """A Packed with the engine's own layout (the geometry as test_gpu_row_stats._twin takes it)."""
    info = eng.info()
    packed = pkg.Packed(m, k=eng.k, nnz_per_lane=info["packet_entries"] // 64, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    return packed


def _expect(pkg, eng, m, allow=None, packed=None):
    packed = packed or _packed_twin(pkg, eng, m)
    want = [pkg.col_stats(m, kind, allow) for kind in KINDS]
    for kind in KINDS:
        assert np.array_equal(_u32(packed.col_stats(kind, allow)), _u32(want[kind])), "the host twin and the COO disagree"
    return want


def _check_engine(pkg, eng, m, label, packed=None):
    want = _expect(pkg, eng, m, None, packed)
    for kind in KINDS:
        got = eng.col_stats(kind)
        assert got.shape == (m.cols,) and got.dtype == (np.uint32 if kind == 0 else np.float32)
        bad = np.flatnonzero(_u32(got) != _u32(want[kind]))
        assert bad.size == 0, f"{label} kind {kind}: {bad.size} columns differ, first {bad[:8]}: {got[bad[:8]]} != {want[kind][bad[:8]]}"
    return want


def _masked(pkg, torch, eng, kind, masks, cols, mask_stride=None, out_gap=0):
    """enqueue_col_stats over len(masks) sets (bool[rows] each; mask_stride=0: masks[0] for every set) into a strided output inside a
    sentinel pattern; returns [sets][cols] words after checking that the gaps and the guard zones are untouched."""
    rows = masks[0].size
    words = np.stack([pkg.row_mask(rows, a) for a in masks])
    n = len(masks)
    d_masks = torch.from_numpy(words.view(np.int32)).cuda()
    stride = cols + out_gap
    buf = torch.full((GUARD + n * stride + GUARD,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_col_stats(kind, buf.data_ptr() + 4 * GUARD, masks=d_masks.data_ptr(), mask_stride=words.shape[1] if mask_stride is None else mask_stride,
                          out_stride=stride, count=n)
    eng.synchronize()
    torch.cuda.synchronize()
    out = buf.cpu().numpy().view(np.uint32)
    assert np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + n * stride:] == SENTINEL), "written outside the sets"
    body = out[GUARD:GUARD + n * stride].reshape(n, stride)
    assert np.all(body[:, cols:] == SENTINEL), "the words between the sets were touched"
    return body[:, :cols]


@pytest.mark.parametrize("nnz_per_lane", [4, 8])
@pytest.mark.parametrize("last_row_empty", [True, False], ids=["last_empty", "last_full"])
def test_edges(pkg, nnz_per_lane, last_row_empty):
    m = _edges(pkg, last_row_empty)[0]
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, nnz_per_lane=nnz_per_lane)
    assert eng.info()["packet_entries"] == 64 * nnz_per_lane
    nnz, cmax, cmin = _check_engine(pkg, eng, m, f"edges C={nnz_per_lane}")
    # row 202 repeats column 950 (counted twice), row 203 holds column 951's only entry, an explicit 0.0; rows 300.. are negative
    assert nnz[950] == np.unique(m.row[m.col == 950]).size + 1 and nnz[951] == 1 and cmin[951] == 0.0 and cmax[951] == 0.0 and cmin[960] == -1.0
    eng.close()


GENERATED = [(2500, 300, 4), (2500, 1024, 4), (2500, 1024, 8), (20000, 4096, 4), (8000, 16384, 4)]


@pytest.mark.parametrize("rows,cols,c_lane", GENERATED)
def test_generated_matrices(pkg, rows, cols, c_lane):
    import torch
    m = signed(pkg, pkg.generate_matrix(rows, cols, 20, "gamma" if cols == 1024 else "uniform", 5 + cols), cols)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, nnz_per_lane=c_lane)
    assert eng.info()["packet_entries"] == 64 * c_lane
    _check_engine(pkg, eng, m, f"{rows}x{cols} C={c_lane}")
    # ... and under a 50 % mask (the FILT instantiations of the tier)
    half = np.random.default_rng(rows).random(m.rows) < 0.5
    for kind in KINDS:
        got = _masked(pkg, torch, eng, kind, [half], m.cols)
        assert np.array_equal(got[0], _u32(pkg.col_stats(m, kind, half))), (cols, c_lane, kind)
    eng.close()


def test_partition_shapes(pkg):
    rng = np.random.default_rng(7)
    rows, per = 128, 8  # 1024 entries: the last row ends on the last slot of a packet, no padding at 4 entries per lane
    fit = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    few = signed(pkg, pkg.generate_matrix(1000, 512, 20, "uniform", 13), 13)  # fewer partitions than waves
    leak = padding_leak_matrix(pkg)
    for label, m in (("exact fit", fit), ("1000x512", few), ("padding leak", leak)):
        for c_lane in (4, 8):
            eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0, nnz_per_lane=c_lane)
            nnz, cmax, cmin = _check_engine(pkg, eng, m, f"{label} C={c_lane}")
            if m is leak:
                assert nnz[0] == 100 and cmin[0] >= 0.25 and cmax[1] < 0 and nnz[63] == 0 and np.isneginf(cmax[63]) and np.isposinf(cmin[63])
                assert int(nnz.sum()) == m.row.size == int(eng.row_stats(pkg._lib.ROW_NNZ).sum())
            eng.close()


def test_long_partitions_and_geometry(pkg):
    import torch
    m = signed(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41)
    packed = pkg.Packed(m, k=16, n_wave_partitions=8)
    assert packed.info()["packets_per_partition"] >= 300
    eng = pkg.SpMV.from_packed(packed, k=16, device=0)
    assert eng.info()["n_wave_partitions"] == 8
    _check_engine(pkg, eng, m, "8 long partitions", packed)
    half = np.random.default_rng(2).random(m.rows) < 0.5
    assert np.array_equal(_masked(pkg, torch, eng, 0, [half], m.cols)[0], pkg.col_stats(m, 0, half))
    eng.close()
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 9), 9)
    for kw in (dict(threads_per_wg=256, waves_per_cu=4), dict(threads_per_wg=64, waves_per_cu=4), dict(waves_per_cu=1)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, **kw)
        _check_engine(pkg, eng, m, f"geometry {kw}")
        eng.close()


def test_lds_contention_and_long_rows(pkg):
    import torch
    m = every_row_matrix(pkg, 20000, 1024)  # column 7 in every row: all 64 lanes hit one LDS word
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    nnz = _check_engine(pkg, eng, m, "one column in every row")[0]
    assert nnz[7] >= m.rows
    eng.close()
    # rows of 700 entries span three packets
    rng = np.random.default_rng(19)
    lens = np.where(np.arange(600) % 50 == 10, 700, rng.integers(0, 12, 600))
    row = np.repeat(np.arange(600), lens)
    m = coo(pkg, 600, 1024, row, rng.integers(0, 1024, row.size), rng.standard_normal(row.size))
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    _check_engine(pkg, eng, m, "rows of 700 entries")
    only = np.arange(m.rows) == 310  # the only allowed row crosses packet boundaries
    for kind in KINDS:
        got = _masked(pkg, torch, eng, kind, [only], m.cols)[0]
        assert np.array_equal(got, _u32(pkg.col_stats(m, kind, only))), kind
    assert int(_masked(pkg, torch, eng, 0, [only], m.cols)[0].sum()) == 700
    eng.close()


def test_masks_shared_per_set_and_strided(pkg):
    import torch
    m = _edges(pkg, False)[0]
    rng = np.random.default_rng(5)
    masks = [rng.random(m.rows) < 0.5, rng.random(m.rows) < 0.001, np.zeros(m.rows, bool), np.ones(m.rows, bool), np.arange(m.rows) == 200]
    for c_lane in (4, 8):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, nnz_per_lane=c_lane)
        packed = _packed_twin(pkg, eng, m)
        for kind in KINDS:
            got = _masked(pkg, torch, eng, kind, masks, m.cols, out_gap=5)
            for i, a in enumerate(masks):
                want = pkg.col_stats(m, kind, a)
                assert np.array_equal(got[i], _u32(want)) and np.array_equal(got[i], _u32(packed.col_stats(kind, a))), (c_lane, kind, i)
            # one mask shared by three sets (mask_stride = 0)
            shared = _masked(pkg, torch, eng, kind, [masks[0]] * 3, m.cols, mask_stride=0, out_gap=1)
            assert all(np.array_equal(shared[i], got[0]) for i in range(3)), (c_lane, kind)
        assert int(_masked(pkg, torch, eng, 0, [masks[4]], m.cols)[0].sum()) == 700
        eng.close()


def test_forty_sets_cross_the_launch_boundary(pkg):
    import torch
    m = signed(pkg, pkg.generate_matrix(2500, 300, 20, "uniform", 3), 3)
    rng = np.random.default_rng(40)
    masks = [rng.random(m.rows) < (i + 1) / 41 for i in range(40)]
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    for kind in KINDS:
        got = _masked(pkg, torch, eng, kind, masks, m.cols, out_gap=20)
        for i, a in enumerate(masks):
            assert np.array_equal(got[i], _u32(pkg.col_stats(m, kind, a))), (kind, i)
    eng.close()


def test_installed_filter_and_state(pkg):
    L = pkg._lib
    m = signed(pkg, pkg.generate_matrix(5000, 512, 20, "uniform", 61), 61)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    with pytest.raises(pkg.TkspmvError) as e:
        eng.col_stats(0, use_filter=True)
    assert e.value.status == L.ERR_STATE
    allow = np.random.default_rng(8).random(m.rows) < 0.3
    eng.set_filter(pkg.row_mask(m.rows, allow))
    for kind in KINDS:
        assert np.array_equal(_u32(eng.col_stats(kind, use_filter=True)), _u32(pkg.col_stats(m, kind, allow))), kind
        assert np.array_equal(_u32(eng.col_stats(kind)), _u32(pkg.col_stats(m, kind))), kind
    eng.close()


def _single_column_clauses(cols_list, n_cols):
    t = np.zeros(n_cols, dtype=np.uint32)
    for b, c in enumerate(cols_list):
        t[c] |= np.uint32(1 << b)
    return t


def test_composition_with_match(pkg):
    """In stream order, nothing waited for in between: match -> its mask -> column counts; and COL_NNZ beside match's counts."""
    import torch
    L = pkg._lib
    m = _edges(pkg, False)[0]
    words = max(1, (m.rows + 31) // 32)
    cols32 = [0, 1023, 950, 951, 952, 953, 960, 970, 980, 10, 20, 30, 40, 45, 60, 100, 105, 107, 200, 300, 400, 500, 600, 700, 800, 899, 5, 961, 971, 981, 965, 975]
    table = _single_column_clauses(cols32, m.cols)
    preds = np.zeros((32, 4), dtype=np.uint32)
    preds[:, 0] = 1 << np.arange(32, dtype=np.uint64)  # query b: must = bit b, the single-column clause {cols32[b]}

    def run(mat):
        eng = pkg.SpMV(mat.row, mat.col, mat.val, mat.rows, mat.cols, k=16, device=0)
        d_table = torch.from_numpy(table.view(np.int32)).cuda()
        d_preds = torch.from_numpy(preds.view(np.int32)).cuda()
        d_masks = torch.zeros((32, words), dtype=torch.int32, device="cuda")
        d_counts = torch.zeros(32, dtype=torch.int32, device="cuda")
        d_nnz = torch.zeros(mat.cols, dtype=torch.int32, device="cuda")
        d_co = torch.zeros(mat.cols, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.enqueue_match(d_table.data_ptr(), d_preds.data_ptr(), 32, d_masks.data_ptr(), out_stride=words, dev_counts=d_counts.data_ptr())
        eng.enqueue_col_stats(L.COL_NNZ, d_nnz.data_ptr())
        eng.enqueue_col_stats(L.COL_NNZ, d_co.data_ptr(), masks=d_masks.data_ptr() + 4 * words * 6)  # the rows that carry column 960
        eng.synchronize()
        torch.cuda.synchronize()
        eng.close()
        return d_counts.cpu().numpy().view(np.uint32), d_nnz.cpu().numpy().view(np.uint32), d_co.cpu().numpy().view(np.uint32)

    # as is: row 202 repeats column 950, so COL_NNZ[950] is larger than the document frequency by exactly that repeat
    df, nnz, co = run(m)
    assert np.array_equal(nnz, pkg.col_stats(m, 0))
    diff = nnz[cols32].astype(np.int64) - df.astype(np.int64)
    assert diff[2] == 1 and not diff[np.arange(32) != 2].any(), diff
    has960 = np.zeros(m.rows, dtype=bool)
    has960[m.row[m.col == 960]] = True
    assert has960.sum() == df[6] > 0 and np.array_equal(co, pkg.col_stats(m, 0, has960)) and co[960] == df[6]
    # with the repeated entry removed, COL_NNZ is the document frequency
    keep = np.ones(m.row.size, dtype=bool)
    keep[np.flatnonzero((m.row == 202) & (m.col == 950))[1]] = False
    df, nnz, _ = run(coo(pkg, m.rows, m.cols, m.row[keep], m.col[keep], m.val[keep]))
    assert np.array_equal(nnz[cols32], df)


def test_scope(pkg, tmp_path):
    m = signed(pkg, pkg.generate_matrix(20000, 1024, 20, "gamma", 9), 9)
    # an engine made from a saved and loaded file: no COO anywhere near it
    packed = pkg.Packed(m, k=16, n_wave_partitions=pkg.Packed.wave_partitions(device=0, m=m))
    packed.save(tmp_path / "m.tkspmv")
    eng = pkg.SpMV.from_packed(pkg.Packed.load(tmp_path / "m.tkspmv"), k=16, device=0)
    want = _check_engine(pkg, eng, m, "from_packed", packed)
    eng.close()
    # first_row: columns are global, the outputs are the same
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, first_row=1000)
    for kind in KINDS:
        assert np.array_equal(_u32(eng.col_stats(kind)), _u32(want[kind])), kind
    eng.close()
    # an approximate per-partition engine is served without a mask; with one it has the filtered path's scope
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    for kind in KINDS:
        assert np.array_equal(_u32(eng.col_stats(kind)), _u32(want[kind])), kind
    eng.set_filter(pkg.row_mask(m.rows))
    with pytest.raises(pkg.TkspmvError) as e:
        eng.col_stats(0, use_filter=True)
    assert e.value.status == pkg._lib.ERR_UNSUPPORTED
    eng.close()


def test_status_codes(pkg):
    import torch
    L = pkg._lib
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    words = (m.rows + 31) // 32
    d_out = torch.full((2 * m.cols,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    d_mask = torch.full((words,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    O, M = d_out.data_ptr(), d_mask.data_ptr()
    h_out = np.full(m.cols, SENTINEL, dtype=np.uint32)

    def status_of(fn):
        try:
            fn()
        except pkg.TkspmvError as e:
            return e.status
        return 0

    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=pkg.F16)
    assert status_of(lambda: eng.enqueue_col_stats(0, O)) == L.ERR_UNSUPPORTED
    assert status_of(lambda: eng.col_stats(1)) == L.ERR_UNSUPPORTED
    assert status_of(lambda: eng.enqueue_col_stats(3, O)) == L.ERR_INVALID  # INVALID comes before UNSUPPORTED
    assert status_of(lambda: eng.enqueue_col_stats(0, 0)) == L.ERR_INVALID
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    for kind in (-1, 3):
        assert status_of(lambda: eng.enqueue_col_stats(kind, O)) == L.ERR_INVALID, kind
        assert L.lib().tkspmv_col_stats(eng._h, kind, 0, h_out.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID, kind
    assert status_of(lambda: eng.enqueue_col_stats(0, 0)) == L.ERR_INVALID
    assert status_of(lambda: eng.enqueue_col_stats(0, O, count=0)) == L.ERR_INVALID
    assert status_of(lambda: eng.enqueue_col_stats(0, O, count=2, out_stride=m.cols)) == L.ERR_INVALID  # no masks: count must be 1
    assert status_of(lambda: eng.enqueue_col_stats(0, O, masks=M, count=2, out_stride=m.cols - 1)) == L.ERR_INVALID
    assert L.lib().tkspmv_col_stats(eng._h, 0, 0, None) == L.ERR_INVALID
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(h_out == SENTINEL) and np.all(d_out.cpu().numpy().view(np.uint32) == SENTINEL), "a rejected call wrote its output"
    eng.enqueue_col_stats(0, O, masks=M, count=2, out_stride=m.cols)
    eng.synchronize()
    torch.cuda.synchronize()
    want = np.bincount(m.col, minlength=m.cols).astype(np.uint32)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), np.concatenate([want, want]))
    eng.close()


def test_engine_state_is_untouched(pkg):
    import torch
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    d_q = torch.from_numpy(xq).cuda()
    d_out = torch.zeros(m.cols, dtype=torch.int32, device="cuda")
    d_idx = [torch.zeros((8, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    d_val = [torch.zeros((8, k), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    # the reference: a batch call alone
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[0].data_ptr(), d_val[0].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    want_idx, want_val = d_idx[0].cpu().numpy().copy(), _u32(d_val[0].cpu().numpy()).copy()
    eng.enqueue_batch(d_q.data_ptr(), 8)  # (engine-owned result pair: the last query wins)
    eng.synchronize()
    res0, counters0 = eng.read_result(), eng.debug_counters()
    for kind in KINDS:
        eng.enqueue_col_stats(kind, d_out.data_ptr())
    eng.synchronize()
    res1, counters1 = eng.read_result(), eng.debug_counters()
    assert counters1 == counters0, "enqueue_col_stats moved a counter"
    assert np.array_equal(res0[1], res1[1]) and np.array_equal(_u32(res0[0]), _u32(res1[0])), "enqueue_col_stats changed the result pair"
    # a batch call right behind an unwaited pass returns the same lists
    d_idx[1].zero_(), d_val[1].zero_()
    torch.cuda.synchronize()
    eng.enqueue_col_stats(1, d_out.data_ptr())
    eng.enqueue_batch(d_q.data_ptr(), 8, d_idx[1].data_ptr(), d_val[1].data_ptr())
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_idx[1].cpu().numpy(), want_idx) and np.array_equal(_u32(d_val[1].cpu().numpy()), want_val)
    eng.close()
