"""Column statistics without a GPU: Packed.col_stats (tkspmv_packed_col_stats, the twin that walks the packed stream) against
host.col_stats (numpy over the COO alone), word for word (COL_NNZ) and bit for bit (COL_MAX, COL_MIN). No tolerance anywhere. Plus
the helpers made of the statistics (idf_weights, score_bound) and the status codes of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from support import coo, signed
from test_gpu_match import _edges
from test_score_rows_host import _hand_made, _words

KINDS = (0, 1, 2)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def padding_leak_matrix(pkg):
    """300 rows x 64 columns, 7 entries per row: column 0 in every third row with values >= 0.25 only, column 1 with negative values
    only, column 63 never used, the rest signed in columns 2..62. 2100 entries never fill a partition's last packet (256 or 512 slots)
    at any of the partition counts used, so the stream ends in padding -- +0.0 at column 0, which would drag MIN[0] to 0, and, counted,
    inflate NNZ[0]."""
    rng = np.random.default_rng(77)
    row, col, val = [], [], []
    for r in range(300):
        c = rng.choice(np.arange(2, 63), 5, replace=False)
        v = rng.standard_normal(5)
        row += [r] * 7
        col += [0 if r % 3 == 0 else int(c[0]), 1] + [int(x) for x in c]
        val += [0.25 + rng.random() if r % 3 == 0 else float(v[0]), -0.1 - rng.random()] + [float(x) for x in v]
    return coo(pkg, 300, 64, row, col, val)


def every_row_matrix(pkg, rows=3000, cols=1024):
    """Column 7 is present in every row (all 64 lanes of a wave meet in one word), beside 9 random columns."""
    rng = np.random.default_rng(11)
    col = rng.integers(0, cols, (rows, 10))
    col[:, 3] = 7
    return coo(pkg, rows, cols, np.repeat(np.arange(rows), 10), col.ravel(), rng.standard_normal(rows * 10))


def _ends_in_padding(packed, c_lane):
    """Number of partitions whose last packet's last slot ends no row: what follows the last row end there is padding."""
    raw = packed.raw()
    fl = _words(raw, c_lane)
    first, count = np.asarray(raw[3]), np.asarray(raw[4])
    return sum(1 for f, n in zip(first, count) if n and not (fl[f + n - 1, -1] & 1))


def _packings(cols):
    """(entries per lane, wave partitions): 4 and, where it exists, 8 entries per lane; many short partitions and 8 long ones."""
    return [(c_lane, parts) for c_lane in ((4, 8) if cols <= 1024 else (4,)) for parts in (8, 64)]


def _compare(pkg, m, packed, allow=None, label=""):
    got = []
    for kind in KINDS:
        want = pkg.col_stats(m, kind, allow)
        have = packed.col_stats(kind, allow)
        assert have.shape == (m.cols,) and have.dtype == want.dtype == (np.uint32 if kind == 0 else np.float32)
        bad = np.flatnonzero(_u32(have) != _u32(want))
        assert bad.size == 0, f"{label} kind {kind}: {bad.size} columns differ, first {bad[:8]}: {have[bad[:8]]} != {want[bad[:8]]}"
        got.append(have)
    return got


def _masks(m, long_row=None):
    rng = np.random.default_rng(m.rows)
    out = {"ones": np.ones(m.rows, bool), "zeros": np.zeros(m.rows, bool), "half": rng.random(m.rows) < 0.5, "rare": rng.random(m.rows) < 0.001}
    if long_row is not None:
        out["one long row"] = np.arange(m.rows) == long_row
    return out


def _matrices(pkg):
    yield "hand-made", _hand_made(pkg, 1024)[0], 6
    for last_row_empty in (False, True):
        yield f"edges last_row_empty={last_row_empty}", _edges(pkg, last_row_empty)[0], 200  # (row 200: 700 entries over three packets)
    yield "padding leak", padding_leak_matrix(pkg), None
    yield "every row", every_row_matrix(pkg), None
    for rows, cols in ((2500, 300), (2500, 1024), (2500, 4096), (3000, 16384)):
        yield f"{rows}x{cols}", signed(pkg, pkg.generate_matrix(rows, cols, 20, "gamma" if cols == 1024 else "uniform", 5 + cols), cols), None


def test_twin_matches_the_coo(pkg):
    for label, m, long_row in _matrices(pkg):
        for c_lane, parts in _packings(m.cols):
            packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=parts)
            assert packed.info()["packet_entries"] == 64 * c_lane
            where = f"{label} C={c_lane} parts={parts}"
            nnz, cmax, cmin = _compare(pkg, m, packed, None, where)
            assert int(nnz.sum(dtype=np.int64)) == m.row.size == int(packed.row_stats(pkg._lib.ROW_NNZ).sum(dtype=np.float64)), where
            empty = nnz == 0
            assert np.all(np.isneginf(cmax[empty])) and np.all(np.isposinf(cmin[empty])) and np.all(cmax[~empty] >= cmin[~empty]), where
            for name, allow in _masks(m, long_row).items():
                got = _compare(pkg, m, packed, allow, f"{where} mask {name}")
                if name == "zeros":
                    assert not got[0].any() and np.all(np.isneginf(got[1])) and np.all(np.isposinf(got[2]))
                if name == "one long row":
                    assert int(got[0].sum()) == np.count_nonzero(m.row == long_row) >= 700
            # mask words are accepted like a bool array
            half = _masks(m)["half"]
            assert np.array_equal(packed.col_stats(0, pkg.row_mask(m.rows, half)), packed.col_stats(0, half))


def test_eight_long_partitions(pkg):
    m = signed(pkg, pkg.generate_matrix(40000, 1024, 20, "gamma", 41), 41)
    packed = pkg.Packed(m, k=16, n_wave_partitions=8)
    assert packed.info()["n_wave_partitions"] == 8 and packed.info()["packets_per_partition"] >= 300
    _compare(pkg, m, packed, None, "8 long partitions")
    _compare(pkg, m, packed, _masks(m)["half"], "8 long partitions, 50 %")


def test_padding_does_not_leak(pkg):
    m = padding_leak_matrix(pkg)
    for c_lane, parts in _packings(m.cols):
        packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=parts)
        assert _ends_in_padding(packed, c_lane) >= 1, "the matrix was meant to leave padding behind a partition's last row"
        assert packed.info()["packed_entries"] > m.row.size and np.array_equal(packed.decode()[1], m.col)
        nnz, cmax, cmin = (packed.col_stats(kind) for kind in KINDS)
        assert nnz[0] == 100 and cmin[0] >= 0.25, (c_lane, parts, nnz[0], cmin[0])
        assert nnz[1] == 300 and cmax[1] < 0
        assert nnz[63] == 0 and np.isneginf(cmax[63]) and np.isposinf(cmin[63])
        assert int(nnz.sum()) == m.row.size == int(packed.row_stats(pkg._lib.ROW_NNZ).sum())


def test_repeats_zeros_and_signed_zero(pkg):
    # a repeated column counts twice, an explicit 0.0 counts, and -0.0 < +0.0 in the order of values
    m = coo(pkg, 4, 8, [0, 0, 1, 2, 2, 3], [3, 3, 5, 6, 6, 5], [1.0, 2.0, 0.0, 0.0, -0.0, -3.0])
    packed = pkg.Packed(m, k=2, n_wave_partitions=1)
    nnz, cmax, cmin = _compare(pkg, m, packed, None, "tiny")
    assert nnz.tolist() == [0, 0, 0, 2, 0, 2, 2, 0]
    assert _u32(cmax[6:7])[0] == 0x00000000 and _u32(cmin[6:7])[0] == 0x80000000
    assert cmax[5] == 0.0 and cmin[5] == -3.0 and cmax[3] == 2.0 and cmin[3] == 1.0


def test_idf_weights(pkg):
    n = 1000
    df = np.array([0, 1, 500, n], dtype=np.uint32)
    for scheme in ("bm25", "smooth"):
        w = pkg.idf_weights(df, n, scheme)
        assert w.dtype == np.float32 and np.all(np.isfinite(w)) and np.all(np.diff(w) < 0), (scheme, w)
    assert pkg.idf_weights(df, n)[0] == np.float32(np.log(1 + (n + 0.5) / 0.5)) and pkg.idf_weights(df, n)[3] == np.float32(np.log(1 + 0.5 / (n + 0.5)))
    assert pkg.idf_weights(df, n, "smooth")[0] == np.float32(np.log(1.0 + n) + 1) and pkg.idf_weights(df, n, "smooth")[3] == np.float32(1.0)
    with pytest.raises(ValueError):
        pkg.idf_weights(df, n, "other")


def test_score_bound(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 300, 20, "uniform", 9), 9)
    key = m.row.astype(np.uint64) * np.uint64(1 << 20) + m.col.astype(np.uint64)
    keep = np.sort(np.unique(key, return_index=True)[1])  # (one entry per (row, column): a bound per column knows nothing of repeats)
    m = coo(pkg, m.rows, m.cols, m.row[keep], m.col[keep], m.val[keep])
    cmax, cmin = pkg.col_stats(m, 1), pkg.col_stats(m, 2)
    rng = np.random.default_rng(3)
    for _ in range(5):
        x = rng.standard_normal(m.cols).astype(np.float32)
        y = np.zeros(m.rows, dtype=np.float64)
        np.add.at(y, m.row.astype(np.int64), m.val.astype(np.float64) * x.astype(np.float64)[m.col])
        bound = pkg.score_bound(x, cmax, cmin)
        assert np.isfinite(bound) and np.all(y <= bound)
    # a column without entries contributes 0
    e = coo(pkg, 2, 3, [0, 1], [0, 0], [2.0, -1.0])
    assert pkg.score_bound(np.array([1.0, 5.0, -5.0]), pkg.col_stats(e, 1), pkg.col_stats(e, 2)) == 2.0
    assert pkg.score_bound(np.array([-1.0, 5.0, -5.0]), pkg.col_stats(e, 1), pkg.col_stats(e, 2)) == 1.0


def test_c_abi(pkg, tmp_path):
    L = pkg._lib
    lib = L.lib()
    m = padding_leak_matrix(pkg)
    packed = pkg.Packed(m, k=8, n_wave_partitions=8)
    out = np.full(m.cols, 0xDEADBEEF, dtype=np.uint32)
    O = out.ctypes.data_as(C.c_void_p)
    assert lib.tkspmv_packed_col_stats(None, 0, None, O) == L.ERR_INVALID
    assert lib.tkspmv_packed_col_stats(packed._h, 0, None, None) == L.ERR_INVALID
    for kind in (-1, 3):
        assert lib.tkspmv_packed_col_stats(packed._h, kind, None, O) == L.ERR_INVALID
    assert lib.tkspmv_enqueue_col_stats(None, 0, 1, None, 0, O, 0, None) == L.ERR_INVALID
    assert lib.tkspmv_col_stats(None, 0, 0, O) == L.ERR_INVALID
    assert np.all(out == 0xDEADBEEF), "a rejected call wrote its output"
    f16 = pkg.Packed(m, k=8, n_wave_partitions=8, precision=pkg.F16)
    assert lib.tkspmv_packed_col_stats(f16._h, 0, None, O) == L.ERR_UNSUPPORTED and np.all(out == 0xDEADBEEF)
    with pytest.raises(pkg.TkspmvError):
        f16.col_stats(0)
    # a saved and loaded file: no COO anywhere near it
    packed.save(tmp_path / "m.tkspmv")
    loaded = pkg.Packed.load(tmp_path / "m.tkspmv")
    half = np.random.default_rng(1).random(m.rows) < 0.5
    for kind in KINDS:
        assert np.array_equal(_u32(loaded.col_stats(kind)), _u32(pkg.col_stats(m, kind)))
        assert np.array_equal(_u32(loaded.col_stats(kind, half)), _u32(pkg.col_stats(m, kind, half)))
    assert lib.tkspmv_packed_col_stats(loaded._h, 0, None, O) == 0 and np.array_equal(out, np.bincount(m.col, minlength=m.cols))
