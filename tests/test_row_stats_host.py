"""Row statistics without a GPU: the symbols of every layer, argument checks that come before any device call, and the claim the
feature rests on -- a row's L1 norm and squared L2 norm are the row's SCORE with every product replaced by |v| or v*v, summed in the
order every streaming path sums in. The existing order-matched oracle pins that order, unchanged: on a matrix whose values are a
function of the column, val[i] = g[col[i]], the query x = g makes every product g*g = v*v bit for bit, and x = sign(g) makes it
|v|, so Packed.row_stats (tkspmv_packed_row_stats) must equal oracle_lib.packed_scores over the whole stream as bits, for EVERY
row. The matrices and packings are those of test_score_rows_host.py. Every such test asserts that some L2SQ differs from the plain
left-to-right fp32 sum of the row's squares: otherwise the inputs would show nothing about the order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from support import bits, coo
from test_score_rows_host import HINTS, ROW_END, SKIP, _every_packing, _hand_made, _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24  # unit roundoff of float32
TINY_ROW, HUGE_ROW = 12, 13  # hand-made rows whose L2SQ is subnormal / +inf
TINY_COLS, HUGE_COLS, FIRST_FREE_COL = range(0, 8), range(10, 18), 20


def _g(cols, seed):
    """Signed, non-zero, standard-normal: the value of column c in the matrices whose values are a function of the column."""
    g = np.random.default_rng(seed).standard_normal(cols).astype(np.float32)
    g[g == 0] = np.float32(0.5)
    return g


def _by_column(pkg, m, g):
    return coo(pkg, m.rows, m.cols, m.row, m.col, g[m.col])


def _sequential_squares(m):
    """Plain left-to-right fp32 sums of the rows' squares."""
    y = np.zeros(m.rows, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        sq = (m.val * m.val).astype(np.float32)
        starts = np.searchsorted(m.row, np.arange(m.rows + 1), side="left")
        for r in range(m.rows):
            acc = np.float32(0.0)
            for p in sq[starts[r]:starts[r + 1]]:
                acc = np.float32(acc + p)
            y[r] = acc
    return y


def _check_all_kinds(pkg, oracle, m, g, packed, c_lane, label):
    """The four kinds of every row against the oracle over the whole stream / the COO's counts / host.inv_l2; returns L2SQ."""
    L = pkg._lib
    raw = packed.raw()
    has = np.zeros(m.rows, dtype=bool)
    has[m.row] = True
    got = {}
    for kind, x in ((L.ROW_L2SQ, g), (L.ROW_L1, np.sign(g).astype(np.float32))):
        got[kind] = packed.row_stats(kind)
        with np.errstate(over="ignore", under="ignore"):
            want, present = oracle.packed_scores(raw, x, m.rows, c_lane)
        assert np.array_equal(present.astype(bool), has), label
        bad = np.flatnonzero(bits(got[kind]) != bits(want))
        assert bad.size == 0, f"{label} kind {kind}: {bad.size} rows differ from the full-stream sums, first {bad[:8]}: {got[kind][bad[:8]]} != {want[bad[:8]]}"
    nnz = packed.row_stats(L.ROW_NNZ)
    assert np.array_equal(nnz, np.bincount(m.row, minlength=m.rows).astype(np.float32)), label
    inv = packed.row_stats(L.ROW_INV_L2)
    assert np.array_equal(bits(inv), bits(pkg.inv_l2(got[L.ROW_L2SQ]))), label
    assert np.all(np.isfinite(inv)), label
    for a in (got[L.ROW_L2SQ], got[L.ROW_L1], nnz, inv):
        assert a.shape == (m.rows,) and a.dtype == np.float32 and np.all(bits(a[~has]) == 0), f"{label}: a row without entries is not +0.0"
    return got[L.ROW_L2SQ]


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    lib = pkg._lib.lib()
    for sym in ("tkspmv_enqueue_row_stats", "tkspmv_row_stats", "tkspmv_packed_row_stats", "tkspmv_set_boost_cosine"):
        assert sym in pkg._lib.EXPORTED_SYMBOLS, sym
        assert f"int {sym}(" in hdr, sym
        assert hasattr(lib, sym), sym
    for i, name in enumerate(("ROW_NNZ", "ROW_L1", "ROW_L2SQ", "ROW_INV_L2")):
        assert getattr(pkg._lib, name) == i and re.search(rf"#define TKSPMV_{name} {i}\b", hdr), name
    for name in ("enqueue_row_stats", "row_stats", "set_cosine"):
        assert callable(getattr(pkg.SpMV, name)), name
    assert callable(pkg.Packed.row_stats) and callable(pkg.inv_l2) and callable(pkg.cosine_spmv) and callable(pkg.cosine_weights)


def test_bad_arguments_fail_before_any_device_call(pkg):
    lib, INVALID = pkg._lib.lib(), pkg._lib.ERR_INVALID
    f32p = C.POINTER(C.c_float)
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    out = np.full(m.rows + 8, -7.0, dtype=np.float32)
    o = out.ctypes.data_as(f32p)
    # a NULL engine: nothing is called on any device (this test runs without one)
    assert lib.tkspmv_enqueue_row_stats(None, 0, C.c_void_p(64), None) == INVALID
    assert lib.tkspmv_row_stats(None, 0, o) == INVALID
    assert lib.tkspmv_set_boost_cosine(None) == INVALID
    packed = pkg.Packed(m, k=8)
    assert lib.tkspmv_packed_row_stats(None, 0, o) == INVALID
    assert lib.tkspmv_packed_row_stats(packed._h, 0, None) == INVALID
    for kind in (-1, 4):
        assert lib.tkspmv_packed_row_stats(packed._h, kind, o) == INVALID, kind
        with pytest.raises(pkg.TkspmvError) as e:
            packed.row_stats(kind)
        assert e.value.status == INVALID
    assert np.all(out == -7.0)  # (nothing is written by a rejected call)
    assert lib.tkspmv_packed_row_stats(packed._h, pkg._lib.ROW_NNZ, o) == 0
    assert np.all(out[:m.rows] != -7.0) and np.all(out[m.rows:] == -7.0)  # exactly rows floats
    packed.close()


def test_other_value_types_are_unsupported(pkg):
    lib, UNSUPPORTED = pkg._lib.lib(), pkg._lib.ERR_UNSUPPORTED
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    out = np.full(m.rows, -7.0, dtype=np.float32)
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        p = pkg.Packed(m, k=8, precision=prec)
        for kind in range(4):
            assert lib.tkspmv_packed_row_stats(p._h, kind, out.ctypes.data_as(C.POINTER(C.c_float))) == UNSUPPORTED, (prec, kind)
        with pytest.raises(pkg.TkspmvError) as e:
            p.row_stats(pkg._lib.ROW_L2SQ)
        assert e.value.status == UNSUPPORTED
        p.close()
    assert np.all(out == -7.0)


def test_inv_l2_finish(pkg):
    s = np.array([0.0, -0.0, np.inf, np.nan, 4.0, 2.0, 1e-40, 1.4e-45, 3.0e38, -1.0], dtype=np.float32)
    w = pkg.inv_l2(s)
    assert w.dtype == np.float32 and np.all(np.isfinite(w))
    assert np.all(bits(w[[0, 1, 2, 3, 9]]) == 0)
    assert w[4] == np.float32(0.5) and bits(w[5:6])[0] == bits(np.float32(1) / np.sqrt(np.float32(2)))[0]
    assert w[6] > 0 and w[7] > 0 and w[8] > 0


@pytest.mark.parametrize("dist", ["uniform", "gamma"])
@pytest.mark.parametrize("cols", [300, 1024, 4096])
def test_every_row_of_generated_matrices(pkg, oracle, dist, cols):
    g = _g(cols, 100 + cols)
    m = _by_column(pkg, pkg.generate_matrix(2500, cols, 20, dist, 5 + cols), g)
    seq = _sequential_squares(m)
    layouts, order_shows = set(), 0
    for packed, c_lane, label in _every_packing(pkg, m, f"{dist} 2500x{cols}", HINTS):
        l2sq = _check_all_kinds(pkg, oracle, m, g, packed, c_lane, label)
        layouts.add(packed.raw()[1] * 2 // (64 * c_lane))  # half bytes per entry
        order_shows += int(np.count_nonzero(bits(l2sq) != bits(seq)))
    # both fp32 layouts are met: 6 bytes per entry (16-bit column words) and, at C = 4 up to 1024 columns, 5.5 (12-bit words)
    assert 12 in layouts and ((11 in layouts) == (cols <= 1024))
    assert order_shows > 0, "every L2SQ equals the left-to-right fp32 sum of its row's squares: the inputs show nothing about the order"


def _hand_made_by_column(pkg, cols):
    """test_score_rows_host.py's 15-row matrix (empty rows in front, in the middle and at the end; rows of exactly 256, 512 and 1500
    entries) with values by column, its columns moved behind FIRST_FREE_COL, plus a row of values near 1e-20 (TINY_ROW: its L2SQ is
    subnormal) and one near 1e25 (HUGE_ROW: its L2SQ is +inf) on columns of their own. Row 14 stays empty: it has no packet."""
    base, lens = _hand_made(pkg, cols)
    g = _g(cols, 77)
    rng = np.random.default_rng(78)
    g[list(TINY_COLS)] = (np.sign(g[list(TINY_COLS)]) * (1.0 + rng.random(len(TINY_COLS))) * 1e-20).astype(np.float32)
    g[list(HUGE_COLS)] = (np.sign(g[list(HUGE_COLS)]) * (1.0 + rng.random(len(HUGE_COLS))) * 1e25).astype(np.float32)
    col = FIRST_FREE_COL + base.col % (cols - FIRST_FREE_COL)
    row = np.concatenate([base.row, np.full(len(TINY_COLS), TINY_ROW), np.full(len(HUGE_COLS), HUGE_ROW)])
    col = np.concatenate([col, np.array(TINY_COLS), np.array(HUGE_COLS)])
    lens = dict(lens)
    lens[TINY_ROW], lens[HUGE_ROW] = len(TINY_COLS), len(HUGE_COLS)
    return coo(pkg, base.rows, cols, row, col, g[col]), g, lens


@pytest.mark.parametrize("cols", [1024, 4096])
def test_hand_made_rows(pkg, oracle, cols):
    L = pkg._lib
    m, g, lens = _hand_made_by_column(pkg, cols)
    seq = _sequential_squares(m)
    for packed, c_lane, label in _every_packing(pkg, m, f"hand-made x{cols}", HINTS):
        l2sq = _check_all_kinds(pkg, oracle, m, g, packed, c_lane, label)
        raw = packed.raw()
        w, pkt_row = _words(raw, c_lane), raw[2]
        # the empty rows inside [0, last stored row] are placeholders in the stream; the trailing one has no packet at all
        assert int(np.count_nonzero(w & SKIP)) == 4 and int(pkt_row.max()) <= HUGE_ROW, label
        for kind in range(4):
            assert np.all(bits(packed.row_stats(kind)[[0, 1, 4, 9, 14]]) == 0), (label, kind)
        nnz = packed.row_stats(L.ROW_NNZ)
        assert all(nnz[r] == n for r, n in lens.items()) and nnz[3] == 256 and nnz[5] == 512 and nnz[6] == 1500, label
        # the 1500-entry row spans three or more packets, one in the middle whole (no row end in it)
        mine = np.flatnonzero(pkt_row == 6)
        assert any(not np.any(w[p] & ROW_END) for p in mine), label
        # a subnormal sum of squares gives a finite weight, an overflowing one the weight 0
        inv = packed.row_stats(L.ROW_INV_L2)
        assert 0 < l2sq[TINY_ROW] < np.finfo(np.float32).tiny and np.isfinite(inv[TINY_ROW]) and inv[TINY_ROW] > 1e19, (label, l2sq[TINY_ROW], inv[TINY_ROW])
        assert np.isposinf(l2sq[HUGE_ROW]) and bits(inv[HUGE_ROW:HUGE_ROW + 1])[0] == 0, (label, l2sq[HUGE_ROW], inv[HUGE_ROW])
        # the long rows' sums are not the left-to-right ones: the wave's order of summation is what was compared
        assert any(bits(l2sq[r:r + 1])[0] != bits(seq[r:r + 1])[0] for r in (3, 5, 6)), label


def test_partition_tails(pkg, oracle):
    """Rows that end on the last slot of a partition's last packet, and the rows right behind a padded partition tail."""
    rows, per = 128, 8  # 1024 entries: four full packets at C = 4, two at C = 8
    rng = np.random.default_rng(7)
    g = _g(512, 70)
    col = rng.integers(0, 512, rows * per)
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), col, g[col])
    seen_full_tail = order_shows = 0
    seq = _sequential_squares(m)
    for packed, c_lane, label in _every_packing(pkg, m, "exact fit", hints=(1, 2, 4)):
        l2sq = _check_all_kinds(pkg, oracle, m, g, packed, c_lane, label)
        order_shows += int(np.count_nonzero(bits(l2sq) != bits(seq)))
        raw = packed.raw()
        w, pf, pc = _words(raw, c_lane), raw[3], raw[4]
        seen_full_tail += sum(1 for q in range(pf.size) if w[int(pf[q] + pc[q] - 1), 64 * c_lane - 1] & ROW_END)
    assert seen_full_tail >= 6, "no partition ended on the last slot of its last packet: the case shows nothing"
    rows, per = 600, 7  # rows of 7 entries never fill a packet exactly; many partitions
    g = _g(300, 71)
    col = rng.integers(0, 300, rows * per)
    m = coo(pkg, rows, 300, np.repeat(np.arange(rows), per), col, g[col])
    seq = _sequential_squares(m)
    for packed, c_lane, label in _every_packing(pkg, m, "padded tails", hints=(64,)):
        PE = 64 * c_lane
        raw = packed.raw()
        w, pf, pc = _words(raw, c_lane), raw[3], raw[4]
        padded = 0
        for q in range(pf.size - 1):
            ends = np.flatnonzero(w[int(pf[q] + pc[q] - 1)] & ROW_END)
            padded += int(ends.size and ends[-1] < PE - 1)
        assert pf.size >= 4 and padded >= 2, "no padded partition tail: the case shows nothing"
        l2sq = _check_all_kinds(pkg, oracle, m, g, packed, c_lane, label)
        order_shows += int(np.count_nonzero(bits(l2sq) != bits(seq)))
    assert order_shows > 0, "every L2SQ equals the left-to-right fp32 sum of its row's squares: the inputs show nothing about the order"


def test_rows_of_a_loaded_file(pkg, oracle, tmp_path):
    g = _g(1024, 90)
    m = _by_column(pkg, pkg.generate_matrix(1500, 1024, 20, "gamma", 9), g)
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    path = tmp_path / "m.tkspmv"
    packed.save(path)
    loaded = pkg.Packed.load(path)
    l2sq = _check_all_kinds(pkg, oracle, m, g, loaded, 4, "loaded file")
    for kind in range(4):
        assert np.array_equal(bits(loaded.row_stats(kind)), bits(packed.row_stats(kind))), kind
    assert np.count_nonzero(bits(l2sq) != bits(_sequential_squares(m))) > 0


@pytest.mark.parametrize("c_lane", [4, 8])
def test_general_matrices_against_float64(pkg, c_lane):
    """Values that are no function of the column, signed: L1 and L2SQ against float64 sums within the textbook bound of a sum of n
    non-negative fp32 terms in any order, n * u / (1 - n * u) relative with u = 2^-24 (each term itself carries one rounding, which
    the bound's n counts: n - 1 additions and one multiplication); INV_L2 against the float64 recipe host.cosine_weights."""
    L = pkg._lib
    g = pkg.generate_matrix(2500, 1024, 20, "gamma", 21)
    sign = np.where(np.random.default_rng(22).random(g.val.size) < 0.5, -1.0, 1.0).astype(np.float32)
    m = coo(pkg, g.rows, g.cols, g.row, g.col, g.val * sign)
    packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=64)
    n = np.bincount(m.row, minlength=m.rows).astype(np.float64)
    assert np.array_equal(packed.row_stats(L.ROW_NNZ), n.astype(np.float32))
    bound = n * EPS / (1.0 - n * EPS)
    v64 = m.val.astype(np.float64)
    l1 = np.bincount(m.row, weights=np.abs(v64), minlength=m.rows)
    l2 = np.bincount(m.row, weights=v64 * v64, minlength=m.rows)
    got_l1, got_l2 = packed.row_stats(L.ROW_L1).astype(np.float64), packed.row_stats(L.ROW_L2SQ).astype(np.float64)
    assert np.all(np.abs(got_l1 - l1) <= bound * l1), float(np.max(np.abs(got_l1 - l1) / np.maximum(l1, 1e-300) - bound))
    assert np.all(np.abs(got_l2 - l2) <= bound * l2), float(np.max(np.abs(got_l2 - l2) / np.maximum(l2, 1e-300) - bound))
    w, want = pkg.inv_l2(packed.row_stats(L.ROW_L2SQ)).astype(np.float64), pkg.cosine_weights(m).astype(np.float64)
    assert np.array_equal(bits(packed.row_stats(L.ROW_INV_L2)), bits(w.astype(np.float32)))
    assert np.all(np.abs(w - want) <= (n / 2 + 3) * EPS * want), float(np.max(np.abs(w - want) / np.maximum(want, 1e-300)) / EPS)
    assert np.all((want == 0) == (n == 0))
    packed.close()
