"""Nearest-n assignment (every stored row's n best-scoring vectors, in order, under an allow-mask) without a GPU: the symbols of every
layer, host.nearest_n and host.margin on hand-made scores, the host twin Packed.nearest (tkspmv_packed_nearest) against
host.nearest_n -- the contract as a stable sort in numpy -- over the order-matched oracle's scores of the whole stream
(oracle_lib.packed_scores), its agreement with Packed.assign, ties, short lists, masks, the ordered labels against float64 scores
from the COO, and the status codes. Values and vectors are signed. Scores are compared as bits."""
import ctypes as C
import os

import numpy as np
import pytest

from support import bits, signed
from test_score_rows_host import _hand_made

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P, F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
NS = (1, 2, 3, 4)
COUNTS = (1, 3, 4, 5, 20)
NONE = 0xFFFFFFFF


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


def _same(got, want, label):
    (gl, gs), (wl, ws) = got, want
    assert gl.dtype == np.uint32 and gs.dtype == np.float32 and gl.shape == gs.shape == wl.shape, label
    bad = np.flatnonzero(np.any((gl != wl) | (bits(gs) != bits(ws)), axis=1))
    assert bad.size == 0, f"{label}: {bad.size} rows differ, first {bad[:4]}: {gl[bad[:4]].tolist()} / {gs[bad[:4]].tolist()} != {wl[bad[:4]].tolist()} / {ws[bad[:4]].tolist()}"


def _oracle_scores(oracle, packed, c_lane, xs, rows):
    raw = packed.raw()
    return np.stack([oracle.packed_scores(raw, x, rows, c_lane)[0] for x in xs])


def _check_against_oracle(pkg, oracle, m, packed, c_lane, xs, label, ns=NS, counts=COUNTS):
    y = _oracle_scores(oracle, packed, c_lane, xs, m.rows)
    for count in counts:
        for n in ns:
            _same(packed.nearest(xs[:count], n), pkg.nearest_n(y[:count], n), f"{label} count={count} n={n}")


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    lib = pkg._lib.lib()
    for sym in ("tkspmv_enqueue_nearest", "tkspmv_nearest", "tkspmv_packed_nearest"):
        assert sym in pkg._lib.EXPORTED_SYMBOLS, sym
        assert f"int {sym}(" in hdr, sym
        assert hasattr(lib, sym), sym
    for name in ("enqueue_nearest", "nearest"):
        assert callable(getattr(pkg.SpMV, name)), name
    assert callable(pkg.Packed.nearest)
    for name in ("nearest_n", "margin", "nearest_spmv"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__, name
    assert pkg.NEAREST_NONE == NONE == pkg._lib.NEAREST_NONE and pkg.NEAREST_MAX_N == 4 == pkg._lib.NEAREST_MAX_N
    assert "#define TKSPMV_NEAREST_MAX_N 4" in hdr and "#define TKSPMV_NEAREST_NONE 0xFFFFFFFFu" in hdr


def test_nearest_n_and_margin_restate_the_contract(pkg):
    ninf = -np.inf
    y = np.array([[1.0, 0.0, -2.0, -0.0, 3.0], [1.0, -0.0, -1.0, 0.0, 2.0], [2.0, 0.0, -1.0, 0.0, 3.0]], dtype=np.float32)
    labels, scores = pkg.nearest_n(y, 4)
    # ties (also +0.0 against -0.0) keep the order of the indices; the fourth entry of three vectors is padding
    assert labels.tolist() == [[2, 0, 1, NONE], [0, 1, 2, NONE], [1, 2, 0, NONE], [0, 1, 2, NONE], [0, 2, 1, NONE]]
    want = np.array([[2, 1, 1, ninf], [0, -0.0, 0, ninf], [-1, -1, -2, ninf], [-0.0, 0, 0, ninf], [3, 3, 2, ninf]], dtype=np.float32)
    assert np.array_equal(bits(scores), bits(want))
    l1, s1 = pkg.nearest_n(y, 1)
    a1, b1 = pkg.nearest(y)
    assert np.array_equal(l1[:, 0], a1) and np.array_equal(bits(s1[:, 0]), bits(b1))
    mask = np.array([True, False, True, False, True])
    lm, sm = pkg.nearest_n(y, 2, mask)
    assert np.all(lm[~mask] == NONE) and np.all(sm[~mask] == ninf)
    assert np.array_equal(lm[mask], labels[mask, :2]) and np.array_equal(bits(sm[mask]), bits(scores[mask, :2]))
    assert pkg.margin(scores).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert np.all(pkg.margin(s1) == np.inf)  # no second entry
    assert np.all(pkg.margin(pkg.nearest_n(y[:1], 3)[1]) == np.inf)  # one vector: the second entry is padding
    assert np.isnan(pkg.margin(sm)[1]) and pkg.margin(sm)[0] == 1.0
    for bad in (lambda: pkg.nearest_n(np.zeros(4, dtype=np.float32), 1), lambda: pkg.nearest_n(y, 0), lambda: pkg.nearest_n(y, 5),
                lambda: pkg.nearest_n(y, 2, np.ones(4, dtype=bool)), lambda: pkg.margin(np.zeros(3, dtype=np.float32))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("dist", ["uniform", "gamma"])
@pytest.mark.parametrize("cols", [300, 1024, 4096])
def test_twin_against_the_contract_on_generated_matrices(pkg, oracle, dist, cols):
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, dist, 5 + cols), cols)
    xs = _xs(20, cols, 200 + cols)
    for packed, c_lane, label in _packings(pkg, m):
        _check_against_oracle(pkg, oracle, m, packed, c_lane, xs, f"{dist} 2500x{cols} {label}")


@pytest.mark.parametrize("cols", [1024, 4096])
def test_twin_against_the_contract_on_hand_made_rows(pkg, oracle, cols):
    """Empty rows in front, in the middle and at the end; rows of 256, 512 and 1500 entries, which span packets."""
    m, lens = _hand_made(pkg, cols)
    xs = _xs(20, cols, 11)
    empty = [r for r in range(m.rows) if r not in lens]
    for packed, c_lane, label in _packings(pkg, m, hints=(1, 7, 4096)):
        _check_against_oracle(pkg, oracle, m, packed, c_lane, xs, f"hand-made x{cols} {label}")
        labels, scores = packed.nearest(xs[:3], 4)  # rows without entries: labels 0, 1, 2 with +0.0f, then padding
        assert np.all(labels[empty] == np.array([0, 1, 2, NONE], dtype=np.uint32)), label
        assert np.all(bits(scores[empty, :3]) == 0) and np.all(scores[empty, 3] == -np.inf), label


def test_n_1_without_a_mask_is_assign(pkg):
    for m in (signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 13), 13), _hand_made(pkg, 1024)[0]):
        for packed, _, label in _packings(pkg, m):
            for count in (1, 5, 20):
                xs = _xs(count, 1024, 14 + count)
                (l1, s1), (la, ba) = packed.nearest(xs, 1), packed.assign(xs)
                assert np.array_equal(l1[:, 0], la) and np.array_equal(bits(s1[:, 0]), bits(ba)), (label, count)


def test_ties(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 13), 13)
    has = np.zeros(m.rows, dtype=bool)
    has[m.row] = True
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    xs = _xs(8, 1024, 14)
    # a vector duplicated at a higher index follows the original directly wherever both are listed, and never precedes it
    dup = xs.copy()
    dup[5] = dup[2]
    labels, scores = packed.nearest(dup, 4)
    r2, j2 = np.nonzero(labels == 2)
    assert r2.size > 0
    inside = j2 < 3
    assert np.all(labels[r2[inside], j2[inside] + 1] == 5) and np.array_equal(bits(scores[r2[inside], j2[inside] + 1]), bits(scores[r2[inside], j2[inside]]))
    r5, j5 = np.nonzero(labels == 5)
    assert np.all(j5 > 0) and np.all(labels[r5, j5 - 1] == 2)
    # all-zero vectors: labels 0 .. n-1 with +0.0f in every row (every product is +-0.0, and a sum that starts at +0.0 stays +0.0)
    for n in NS:
        l0, s0 = packed.nearest(np.zeros((5, 1024), dtype=np.float32), n)
        assert np.all(l0 == np.arange(n, dtype=np.uint32)) and np.all(bits(s0) == 0), n
    # x and -x on rows of one entry: the scores are +-|v x| or, where x is zero at the column, +0.0 and -0.0, which tie: label 0 first
    one = pkg.CooMatrix(rows=64, cols=1024, row=np.arange(64, dtype=np.uint32), col=np.arange(64, dtype=np.uint32), val=np.ones(64, dtype=np.float32))
    x = _xs(1, 1024, 15)[0]
    x[:32] = 0.0
    lz, sz = pkg.Packed(one, k=4).nearest(np.stack([x, -x]), 2)
    assert np.all(lz[:32] == np.array([0, 1], dtype=np.uint32)) and np.all(sz[:32] == 0)  # (whatever the sign of either zero)
    assert np.all(sz[32:, 0] > 0) and np.array_equal(sz[32:, 0], -sz[32:, 1]) and np.array_equal(lz[32:, 0], (x[32:64] < 0).astype(np.uint32))


def test_short_lists(pkg):
    m = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 23), 23)
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    xs = _xs(3, 1024, 24)
    full_l, full_s = packed.nearest(xs, 3)
    for count in (1, 2, 3):
        labels, scores = packed.nearest(xs[:count], 4)
        assert np.all(labels[:, count:] == NONE) and np.all(scores[:, count:] == -np.inf), count
        assert np.all(labels[:, :count] < count) and np.all(np.isfinite(scores[:, :count])), count
    labels, scores = packed.nearest(xs, 4)
    assert np.array_equal(labels[:, :3], full_l) and np.array_equal(bits(scores[:, :3]), bits(full_s))


def test_masks(pkg):
    m, lens = _hand_made(pkg, 1024)
    big = signed(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 33), 33)
    for mat in (m, big):
        packed = pkg.Packed(mat, k=8, n_wave_partitions=7)
        xs = _xs(6, 1024, 34)
        rng = np.random.default_rng(35)
        one = np.zeros(mat.rows, dtype=bool)
        one[mat.rows // 2] = True
        for n in (1, 3, 4):
            plain = packed.nearest(xs, n)
            _same(packed.nearest(xs, n, np.ones(mat.rows, dtype=bool)), plain, "all ones")
            _same(packed.nearest(xs, n, pkg.row_mask(mat.rows)), plain, "all ones as words")
            for name, mask in (("half", rng.random(mat.rows) < 0.5), ("one row", one), ("none", np.zeros(mat.rows, dtype=bool))):
                labels, scores = packed.nearest(xs, n, mask)
                assert np.all(labels[~mask] == NONE) and np.all(scores[~mask] == -np.inf), (name, n)
                assert np.array_equal(labels[mask], plain[0][mask]) and np.array_equal(bits(scores[mask]), bits(plain[1][mask])), (name, n)
        with pytest.raises(ValueError):
            packed.nearest(xs, 2, np.ones(mat.rows + 1, dtype=bool))


@pytest.mark.parametrize("cols", [300, 1024, 4096])
def test_ordered_labels_against_float64_from_the_coo(pkg, cols):
    """Independent of every packed layout: scores from the COO in float64. fp32 products and sums in ANY order stay within
    nnz 2^-24 sum|v x_q| of the exact score, so two vectors whose float64 scores are further apart than
    2 nnz 2^-24 max_q sum|v x_q| cannot be reordered by any fp32 evaluation. A row is DECIDED when that holds for the four gaps among
    its ranks 1 .. 5: its first four labels are then fixed. On decided rows the labels must be equal; and the input (unit rows of 20
    entries, 20 standard-normal vectors) is such that at least 90 % of the non-empty rows are decided -- a condition on the input,
    not a tolerance."""
    count = 20
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, "gamma", 21), 21)
    xs = _xs(count, cols, 22)
    prod = m.val.astype(np.float64)[None, :] * xs.astype(np.float64)[:, m.col]  # [count, nnz]
    y = np.zeros((count, m.rows))
    mag = np.zeros((count, m.rows))
    for q in range(count):
        np.add.at(y[q], m.row, prod[q])
        np.add.at(mag[q], m.row, np.abs(prod[q]))
    nnz = np.bincount(m.row, minlength=m.rows).astype(np.float64)
    order = np.argsort(-y, axis=0, kind="stable")  # [count, rows]
    srt = np.take_along_axis(y, order, axis=0)
    bound = nnz * 2.0 ** -24 * mag.max(axis=0)
    decided = (nnz > 0) & np.all(srt[0:4] - srt[1:5] > 2.0 * bound, axis=0)
    share = np.count_nonzero(decided) / np.count_nonzero(nnz > 0)
    assert share >= 0.9, f"only {share:.4f} of the non-empty rows are decided in float64"
    want = order[:4].T.astype(np.uint32)
    for packed, c_lane, label in _packings(pkg, m):
        for n in NS:
            labels, scores = packed.nearest(xs, n)
            assert np.array_equal(labels[decided], want[decided, :n]), (label, n)
            assert np.all(np.abs(scores[decided] - srt[:n].T[decided]) <= bound[decided, None] + 1e-30), (label, n)


def test_rows_of_a_loaded_file(pkg, tmp_path):
    m = signed(pkg, pkg.generate_matrix(1500, 1024, 20, "gamma", 9), 9)
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    packed.save(tmp_path / "m.tkspmv")
    loaded = pkg.Packed.load(tmp_path / "m.tkspmv")
    xs = _xs(7, 1024, 10)
    _same(loaded.nearest(xs, 3), packed.nearest(xs, 3), "loaded file")


def test_status_codes_of_the_twin_and_checks_before_any_device_call(pkg):
    lib = pkg._lib.lib()
    INVALID, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    xs = _xs(2, 64, 1)
    labels = np.full((m.rows, 4), 0xAAAAAAAA, dtype=np.uint32)
    scores = np.full((m.rows, 4), -7.0, dtype=np.float32)
    X, Lb, S = xs.ctypes.data_as(F32P), labels.ctypes.data_as(U32P), scores.ctypes.data_as(F32P)
    # a NULL engine: INVALID, from both entry points (no engine, hence no device, is ever touched)
    assert lib.tkspmv_enqueue_nearest(None, C.c_void_p(64), 1, 1, None, C.c_void_p(64), C.c_void_p(64), None) == INVALID
    assert lib.tkspmv_nearest(None, X, 2, 1, 0, Lb, S) == INVALID
    packed = pkg.Packed(m, k=8)
    assert lib.tkspmv_packed_nearest(None, X, 2, 2, None, Lb, S) == INVALID
    assert lib.tkspmv_packed_nearest(packed._h, None, 2, 2, None, Lb, S) == INVALID
    assert lib.tkspmv_packed_nearest(packed._h, X, 2, 2, None, None, S) == INVALID
    assert lib.tkspmv_packed_nearest(packed._h, X, 2, 2, None, Lb, None) == INVALID
    for count in (0, -1):
        assert lib.tkspmv_packed_nearest(packed._h, X, count, 2, None, Lb, S) == INVALID, count
    for n in (0, -1, 5):
        assert lib.tkspmv_packed_nearest(packed._h, X, 2, n, None, Lb, S) == INVALID, n
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        p = pkg.Packed(m, k=8, precision=prec)
        assert lib.tkspmv_packed_nearest(p._h, X, 2, 2, None, Lb, S) == UNSUPPORTED, prec
        with pytest.raises(pkg.TkspmvError) as e:
            p.nearest(xs, 2)
        assert e.value.status == UNSUPPORTED
        p.close()
    assert np.all(labels == 0xAAAAAAAA) and np.all(scores == -7.0), "a rejected call wrote its output"
    assert lib.tkspmv_packed_nearest(packed._h, X, 2, 4, None, Lb, S) == 0 and not np.any(labels == 0xAAAAAAAA) and not np.any(scores == -7.0)
    with pytest.raises(pkg.TkspmvError) as e:
        packed.nearest(xs, 5)
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        packed.nearest(xs[:, :-1], 2)
    with pytest.raises(ValueError):
        packed.nearest(np.zeros((0, 64), dtype=np.float32), 2)
