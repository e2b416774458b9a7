"""Assignment (every stored row's best-scoring vector) without a GPU: the symbols of every layer, the argument checks that come
before any device call, and the host twin Packed.assign (tkspmv_packed_assign) against three expectations that share nothing with
it: host.nearest -- the contract's loop in numpy -- over the order-matched oracle's scores of the whole stream
(oracle_lib.packed_scores), one vector at a time; Packed.score_rows of the winning vector; and, from the COO in float64, the labels
of every row whose margin between best and second best is larger than anything fp32 summation can move. Values and vectors are
signed. Everything is compared as bits unless a test says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

from support import bits, coo, signed
from test_score_rows_host import _hand_made

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P, F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float)


def _xs(count, cols, seed):
    return np.random.default_rng(seed).standard_normal((count, cols)).astype(np.float32)


def _packings(pkg, m, hints=(7, 64)):
    for c_lane in (4, 8):
        if c_lane == 8 and m.cols > 1024:  # (8 entries per lane exist up to 1024 columns)
            continue
        for hint in hints:
            packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=hint)
            yield packed, c_lane, f"C={c_lane} hint={hint}"
            packed.close()


def _check_against_oracle(pkg, oracle, m, packed, c_lane, xs, label):
    """Packed.assign(xs) == host.nearest over the oracle's full-stream scores of every vector; best == score_rows of the winner."""
    labels, best = packed.assign(xs)
    assert labels.dtype == np.uint32 and best.dtype == np.float32 and labels.shape == best.shape == (m.rows,), label
    raw = packed.raw()
    y = np.stack([oracle.packed_scores(raw, x, m.rows, c_lane)[0] for x in xs])
    want_labels, want_best = pkg.nearest(y)
    bad = np.flatnonzero((labels != want_labels) | (bits(best) != bits(want_best)))
    assert bad.size == 0, f"{label}: {bad.size} rows differ from nearest(oracle scores), first {bad[:8]}: {labels[bad[:8]]} / {best[bad[:8]]} != {want_labels[bad[:8]]} / {want_best[bad[:8]]}"
    for q in range(xs.shape[0]):  # the winner's score is the score the scoring twin reports for that row and vector
        rows_q = np.flatnonzero(labels == q).astype(np.uint32)
        if rows_q.size:
            assert np.array_equal(bits(packed.score_rows(xs[q], rows_q)), bits(best[rows_q])), (label, q)
    return labels, best


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    lib = pkg._lib.lib()
    for sym in ("tkspmv_enqueue_assign", "tkspmv_assign", "tkspmv_packed_assign"):
        assert sym in pkg._lib.EXPORTED_SYMBOLS, sym
        assert f"int {sym}(" in hdr, sym
        assert hasattr(lib, sym), sym
    for name in ("enqueue_assign", "assign"):
        assert callable(getattr(pkg.SpMV, name)), name
    assert callable(pkg.Packed.assign)
    for name in ("nearest", "assign_spmv"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__, name


def test_nearest_restates_the_contract_loop(pkg):
    y = np.array([[1.0, 0.0, -2.0, -0.0, 3.0], [1.0, -0.0, -1.0, 0.0, 2.0], [2.0, 0.0, -1.0, 0.0, 3.0]], dtype=np.float32)
    labels, best = pkg.nearest(y)
    assert labels.tolist() == [2, 0, 1, 0, 0]  # ties (also +0.0 against -0.0) go to the smallest index
    assert np.array_equal(bits(best), bits(np.array([2.0, 0.0, -1.0, -0.0, 3.0], dtype=np.float32)))
    with pytest.raises(ValueError):
        pkg.nearest(np.zeros(4, dtype=np.float32))


@pytest.mark.parametrize("dist", ["uniform", "gamma"])
@pytest.mark.parametrize("cols", [300, 1024, 4096])
def test_twin_against_the_oracle_on_generated_matrices(pkg, oracle, dist, cols):
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, dist, 5 + cols), cols)
    xs = _xs(5, cols, 200 + cols)
    seen = set()
    for packed, c_lane, label in _packings(pkg, m):
        labels, _ = _check_against_oracle(pkg, oracle, m, packed, c_lane, xs, f"{dist} 2500x{cols} {label}")
        seen.update(labels.tolist())
    assert seen == set(range(5)), "some vector never wins: the inputs show nothing about it"


@pytest.mark.parametrize("cols", [1024, 4096])
def test_twin_against_the_oracle_on_hand_made_rows(pkg, oracle, cols):
    """Empty rows in front, in the middle and at the end; rows of 256, 512 and 1500 entries, which span packets: a carry per vector."""
    m, lens = _hand_made(pkg, cols)
    xs = _xs(6, cols, 11)
    for packed, c_lane, label in _packings(pkg, m, hints=(1, 7, 4096)):
        labels, best = _check_against_oracle(pkg, oracle, m, packed, c_lane, xs, f"hand-made x{cols} {label}")
        empty = [r for r in range(m.rows) if r not in lens]
        assert np.all(labels[empty] == 0) and np.all(bits(best[empty]) == 0), label  # label 0 and the bits of +0.0f
        assert len(set(labels[sorted(lens)].tolist())) >= 3, label


def test_rules(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 13), 13)
    has = np.zeros(m.rows, dtype=bool)
    has[m.row] = True
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    xs = _xs(8, 1024, 14)
    labels, best = packed.assign(xs)
    # a duplicated vector never wins under its larger index
    dup = xs.copy()
    dup[5] = dup[2]
    l2, b2 = packed.assign(dup)
    assert not np.any(l2 == 5) and np.any(l2 == 2)
    assert np.all(l2[labels == 2] == 2) and np.array_equal(bits(b2[labels == 2]), bits(best[labels == 2]))
    # all-zero vectors: every row label 0, +0.0f (every product is +-0.0, and a sum that starts at +0.0 stays +0.0)
    l0, b0 = packed.assign(np.zeros((3, 1024), dtype=np.float32))
    assert np.all(l0 == 0) and np.all(bits(b0) == 0)
    # strictly negative vectors on a positive matrix: every non-empty row's best is negative (a running best that starts at 0 fails)
    pos = coo(pkg, m.rows, m.cols, m.row, m.col, np.abs(m.val) + np.float32(0.01))
    p_pos = pkg.Packed(pos, k=8, n_wave_partitions=64)
    neg = -(np.abs(_xs(4, 1024, 15)) + np.float32(0.01))
    ln, bn = p_pos.assign(neg)
    assert np.all(bn[has] < 0) and len(set(ln[has].tolist())) == 4
    # rows without entries: label 0 and bits 0
    assert np.count_nonzero(~has) == 0 or (np.all(ln[~has] == 0) and np.all(bits(bn[~has]) == 0))
    hm, lens = _hand_made(pkg, 1024)
    lh, bh = pkg.Packed(hm, k=4).assign(-np.abs(_xs(3, 1024, 16)) - 1)
    empty = [r for r in range(hm.rows) if r not in lens]
    assert np.all(lh[empty] == 0) and np.all(bits(bh[empty]) == 0)
    # one vector: label 0 everywhere, best = the row's score
    l1, b1 = packed.assign(xs[3])
    assert np.all(l1 == 0) and np.array_equal(bits(b1), bits(packed.score_rows(xs[3], np.arange(m.rows))))


def test_labels_against_float64_from_the_coo(pkg):
    """Independent of every packed layout: scores from the COO in float64. A row is DECIDED when its float64 margin between best and
    second best exceeds 2 n 2^-24 max_q sum|v x_q| (n the row's entries): fp32 products and sums in ANY order stay within n 2^-24
    sum|v x_q| of the exact score, so no fp32 evaluation can flip the winner. On decided rows the labels must be equal; and the
    input is such that at least 90 % of the non-empty rows are decided (a condition on the input, not a tolerance)."""
    count = 8
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 21), 21)
    xs = _xs(count, 1024, 22)
    prod = m.val.astype(np.float64)[None, :] * xs.astype(np.float64)[:, m.col]  # [count, nnz]
    y = np.zeros((count, m.rows))
    mag = np.zeros((count, m.rows))
    for q in range(count):
        np.add.at(y[q], m.row, prod[q])
        np.add.at(mag[q], m.row, np.abs(prod[q]))
    n = np.bincount(m.row, minlength=m.rows).astype(np.float64)
    srt = np.sort(y, axis=0)
    margin = srt[-1] - srt[-2]
    decided = (n > 0) & (margin > 2.0 * n * 2.0 ** -24 * mag.max(axis=0))
    share = np.count_nonzero(decided) / np.count_nonzero(n > 0)
    assert share >= 0.9, f"only {share:.3f} of the non-empty rows are decided in float64"
    want = np.argmax(y, axis=0).astype(np.uint32)
    for packed, c_lane, label in _packings(pkg, m):
        labels, best = packed.assign(xs)
        assert np.array_equal(labels[decided], want[decided]), label
        assert np.all(np.abs(best[decided] - srt[-1][decided]) <= n[decided] * 2.0 ** -24 * mag.max(axis=0)[decided] + 1e-30), label


def test_rows_of_a_loaded_file(pkg, tmp_path):
    m = signed(pkg, pkg.generate_matrix(1500, 1024, 20, "gamma", 9), 9)
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    packed.save(tmp_path / "m.tkspmv")
    loaded = pkg.Packed.load(tmp_path / "m.tkspmv")
    xs = _xs(7, 1024, 10)
    a, b = packed.assign(xs), loaded.assign(xs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_argument_checks_come_before_any_device_call(pkg):
    lib = pkg._lib.lib()
    INVALID, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    xs = _xs(2, 64, 1)
    labels = np.full(m.rows, 0xAAAAAAAA, dtype=np.uint32)
    best = np.full(m.rows, -7.0, dtype=np.float32)
    X, Lb, B = xs.ctypes.data_as(F32P), labels.ctypes.data_as(U32P), best.ctypes.data_as(F32P)
    # a NULL engine: INVALID, from both entry points (no engine, hence no device, is ever touched)
    assert lib.tkspmv_enqueue_assign(None, C.c_void_p(64), 1, C.c_void_p(64), C.c_void_p(64), None) == INVALID
    assert lib.tkspmv_assign(None, X, 2, Lb, B) == INVALID
    packed = pkg.Packed(m, k=8)
    assert lib.tkspmv_packed_assign(None, X, 2, Lb, B) == INVALID
    assert lib.tkspmv_packed_assign(packed._h, None, 2, Lb, B) == INVALID
    assert lib.tkspmv_packed_assign(packed._h, X, 2, None, B) == INVALID
    assert lib.tkspmv_packed_assign(packed._h, X, 0, Lb, B) == INVALID and lib.tkspmv_packed_assign(packed._h, X, -1, Lb, B) == INVALID
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        p = pkg.Packed(m, k=8, precision=prec)
        assert lib.tkspmv_packed_assign(p._h, X, 2, Lb, B) == UNSUPPORTED, prec
        with pytest.raises(pkg.TkspmvError) as e:
            p.assign(xs)
        assert e.value.status == UNSUPPORTED
        p.close()
    assert np.all(labels == 0xAAAAAAAA) and np.all(best == -7.0), "a rejected call wrote its output"
    assert lib.tkspmv_packed_assign(packed._h, X, 2, Lb, None) == 0 and np.all(labels < 2) and np.all(best == -7.0)  # best may be NULL
    assert lib.tkspmv_packed_assign(packed._h, X, 2, Lb, B) == 0 and not np.any(best == -7.0)
    with pytest.raises(ValueError):
        packed.assign(xs[:, :-1])
    with pytest.raises(ValueError):
        packed.assign(np.zeros((0, 64), dtype=np.float32))
