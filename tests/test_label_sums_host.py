"""Label sums (per-label column sums of the stored rows as 64-bit fixed-point integers) without a GPU: the symbols of every layer,
quantise on hand-made values and against exact rational arithmetic, and the host twin Packed.label_sums (tkspmv_packed_label_sums)
against host.label_sums -- the contract from the COO in numpy int64, which shares nothing with any layout --, exactly: integers have
no tolerance. Then the closing rules as bits, the default exponent, the derived bound against float64 column sums, and the
assign + label_sums chain of spherical k-means."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from support import bits, coo, signed
from test_col_stats_host import _ends_in_padding
from test_score_rows_host import _hand_made

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P, F32P, I64P = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
BINS = (1, 2, 8, 9, 17)


def _wide(pkg, m, seed):
    """The matrix with random signs, every value scaled by a power of two 2^0 .. 2^-20 (so that coarse grids round), and about one
    entry in twelve moved to the column of the entry in front of it in the same row (a column repeated within a row)."""
    rng = np.random.default_rng(seed)
    m = signed(pkg, m, seed)
    val = np.ldexp(m.val, -rng.integers(0, 21, m.val.size).astype(np.int32)).astype(np.float32)
    col = m.col.copy()
    rep = np.flatnonzero((rng.random(col.size) < 1 / 12) & (np.arange(col.size) > 0))
    rep = rep[m.row[rep] == m.row[rep - 1]]
    col[rep] = col[rep - 1]
    return coo(pkg, m.rows, m.cols, m.row, col, val)


def _matrices(pkg):
    for cols in (300, 1024, 4096):
        for dist in ("gamma", "uniform"):
            yield f"{dist} 2500x{cols}", _wide(pkg, pkg.generate_matrix(2500, cols, 20, dist, 7 + cols), cols)
    yield "uniform 600x5000", _wide(pkg, pkg.generate_matrix(600, 5000, 20, "uniform", 31), 31)
    for cols in (1024, 4096):
        yield f"hand-made x{cols}", _hand_made(pkg, cols)[0]


def _packings(pkg, m, hints=(7, 64)):
    for c_lane in (4, 8):
        if c_lane == 8 and m.cols > 1024:  # (8 entries per lane exist up to 1024 columns)
            continue
        for hint in hints:
            packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=hint)
            yield packed, f"C={c_lane} hint={hint}"
            packed.close()


def _labels(rows, n_bins, seed):
    """Random labels in [0, n_bins + 2): about 2 in n_bins + 2 rows have no bin."""
    return np.random.default_rng(seed).integers(0, n_bins + 2, rows).astype(np.uint32)


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    lib = pkg._lib.lib()
    for sym in ("tkspmv_enqueue_label_sums", "tkspmv_enqueue_sums_close", "tkspmv_sums_exponent", "tkspmv_label_sums", "tkspmv_packed_label_sums",
                "tkspmv_packed_sums_exponent", "tkspmv_sums_close_host"):
        assert sym in pkg._lib.EXPORTED_SYMBOLS, sym
        assert f"int {sym}(" in hdr, sym
        assert hasattr(lib, sym), sym
    for name in ("enqueue_label_sums", "enqueue_sums_close", "sums_exponent", "label_sums", "kmeans"):
        assert callable(getattr(pkg.SpMV, name)), name
    assert callable(pkg.Packed.label_sums) and callable(pkg.Packed.sums_exponent)
    for name in ("quantise", "label_sums", "sums_exponent", "close_sums", "kmeans_spmv"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__, name
    assert (pkg._lib.SUMS_RAW, pkg._lib.SUMS_FLOAT, pkg._lib.SUMS_UNIT) == (0, 1, 2)
    for name, value in (("TKSPMV_SUMS_ACCUMULATE", "1u"), ("TKSPMV_SUMS_SINK_LDS", "2u"), ("TKSPMV_SUMS_SINK_DIRECT", "4u")):
        assert f"#define {name} {value}" in hdr, name


def _both(pkg, v, e):
    """quantise(v, e) from numpy and from the library's own function, which must agree."""
    v = np.float32(v)
    q = int(pkg.quantise(np.array([v], dtype=np.float32), e)[0])
    assert q == int(pkg._lib.lib().tkspmv_quantise(int(v.view(np.uint32)), int(e))), (v, e)
    return q


def test_quantise_on_hand_made_values(pkg):
    tiny = np.ldexp(np.float32(1), -149)  # the smallest subnormal
    up = np.nextafter(np.float32(2.5), np.float32(3))
    cases = [
        (1.0, -30, 1 << 30), (1.0, -23, 1 << 23), (3.0, -60, 3 << 60), (1.0, -61, 1 << 61),  # left shifts (s = 7, 0, 38, 38)
        (1.0, -10, 1024), (1.0, 0, 1), (1.75, -1, 4), (1.25, -1, 2), (0.75, 0, 1), (0.25, 0, 0),  # right shifts; 3.5 -> 4 and 2.5 -> 2 are ties
        (0.5, 0, 0), (1.5, 0, 2), (2.5, 0, 2), (3.5, 0, 4), (up, 0, 3),  # exact halves land on the even neighbour, one ulp more goes up
        (-0.5, 0, 0), (-1.5, 0, -2), (-2.5, 0, -2), (-3.5, 0, -4), (-up, 0, -3),
        (tiny, -149, 1), (tiny, -148, 0), (3 * tiny, -148, 2), (-3 * tiny, -148, -2), (5 * tiny, -148, 2), (tiny, -150, 2),  # subnormals
        (0.0, -40, 0), (-0.0, -40, 0), (0.0, 100, 0),
        (1.0, 41, 0), (1.0, 1000, 0), (-1.0, 2 ** 31 - 1, 0),  # shifts of 64 and far more
        (np.finfo(np.float32).max, 128, 1), (np.finfo(np.float32).max, 129, 0), (np.finfo(np.float32).max, 168, 0),  # shifts of 24 (0.99.. -> 1), 25, 64
    ]
    for v, e, want in cases:
        assert _both(pkg, v, e) == want, (v, e, want)
        assert _both(pkg, -np.float32(v), e) == -want, (v, e)


def test_quantise_against_exact_rationals(pkg):
    """round-half-even of v / 2^E in exact rational arithmetic (Python rounds a Fraction to even), wherever the call is defined."""
    rng = np.random.default_rng(5)
    v = np.concatenate([np.ldexp(rng.standard_normal(400), rng.integers(-30, 10, 400)).astype(np.float32),
                        (rng.integers(-64, 64, 200) / 8).astype(np.float32),  # many exact halves
                        np.ldexp(rng.integers(-9, 9, 50).astype(np.float32), -149)])  # subnormals
    for e in (-40, -12, -3, 0, 2, -150):
        ok = (np.frexp(np.abs(v).astype(np.float64))[1] - 24 - e <= 38) | (v == 0)
        got = pkg.quantise(v, e)
        lib = pkg._lib.lib()
        for x, g in zip(v[ok].tolist(), got[ok].tolist()):
            f = Fraction(x) / (Fraction(2) ** e)
            want = round(abs(f)) * (1 if f >= 0 else -1)  # (ties to even on the MAGNITUDE)
            assert g == want, (x, e, g, want)
            assert lib.tkspmv_quantise(int(np.float32(x).view(np.uint32)), e) == want, (x, e)
        assert np.array_equal(pkg.quantise(-v, e)[ok], -got[ok])


def test_twin_equals_the_contract_from_the_coo(pkg):
    """int64 == int64 on every matrix, packing and bin count: the default exponent (every value exact) and two coarse grids (E = -12:
    every value below 2^11 quanta, most of them rounded; E = -3: most values round to 0 or +-1)."""
    for name, m in _matrices(pkg):
        exps = (pkg.sums_exponent(m), -12, -3)
        want = {(n_bins, e): pkg.label_sums(m, _labels(m.rows, n_bins, n_bins), n_bins, e) for n_bins in BINS for e in exps}
        rounded = pkg.quantise(m.val, -12).astype(np.float64) * 2.0 ** -12 != m.val.astype(np.float64)
        assert name.startswith("hand-made") or np.count_nonzero(rounded) > m.val.size // 2, "the coarse grid rounds too few values to show anything"
        for packed, label in _packings(pkg, m, hints=(1, 7, 4096) if name.startswith("hand-made") else (7, 64)):
            for (n_bins, e), w in want.items():
                sums, none = packed.label_sums(_labels(m.rows, n_bins, n_bins), n_bins, e)
                assert none is None and sums.dtype == np.int64 and sums.shape == (n_bins, m.cols)
                bad = np.argwhere(sums != w)
                assert bad.size == 0, f"{name} {label} n_bins={n_bins} E={e}: {len(bad)} words differ, first {bad[:4].tolist()}"


def test_repeats_explicit_zeros_and_labels_without_a_bin(pkg):
    m = coo(pkg, 5, 8, [0, 0, 1, 2, 2, 3, 4], [3, 3, 5, 6, 6, 5, 3], [1.0, 2.0, 0.0, 0.5, -0.0, -3.0, 8.0])
    packed = pkg.Packed(m, k=2, n_wave_partitions=1)
    sums, _ = packed.label_sums([0, 1, 0, 1, 7], 2, -1)
    assert sums[0].tolist() == [0, 0, 0, 6, 0, 0, 1, 0] and sums[1].tolist() == [0, 0, 0, 0, 0, -6, 0, 0]  # (row 4, label 7: no bin)
    assert np.array_equal(sums, pkg.label_sums(m, [0, 1, 0, 1, 7], 2, -1))


def test_padding_never_reaches_column_0(pkg):
    """A matrix with no entry in column 0 whose stream ends in padding (padding looks like +0.0 at column 0, and its row index lies
    beyond the partition's rows): with a coarse grid nothing changes (0 quantises to 0), so the check is that the word stays 0 AND
    that every other word is right with labels that give the rows behind the last one a bin."""
    rng = np.random.default_rng(3)
    rows = 300
    col = np.stack([rng.choice(np.arange(1, 64), 7, replace=False) for _ in range(rows)]).ravel()
    m = coo(pkg, rows, 64, np.repeat(np.arange(rows), 7), col, rng.standard_normal(rows * 7) + 3.0)
    for c_lane in (4, 8):
        for hint in (1, 8):
            packed = pkg.Packed(m, k=4, nnz_per_lane=c_lane, n_wave_partitions=hint)
            assert _ends_in_padding(packed, c_lane) > 0, "the stream does not end in padding: the test shows nothing"
            for n_bins in (1, 3):
                lab = np.arange(rows, dtype=np.uint32) % n_bins
                sums, _ = packed.label_sums(lab, n_bins, -20)
                assert np.all(sums[:, 0] == 0) and np.array_equal(sums, pkg.label_sums(m, lab, n_bins, -20))
                assert np.all(sums[:, 1:].sum(axis=0) > 0)
            packed.close()


def test_closing_rules_as_bits(pkg):
    m = _wide(pkg, pkg.generate_matrix(2500, 1000, 20, "gamma", 8), 8)  # (1000 columns: the last partials are shorter)
    lab = _labels(m.rows, 6, 1)
    lab[lab == 3] = 4  # bin 3 stays empty
    packed = pkg.Packed(m, k=8, n_wave_partitions=16)
    FLOAT, UNIT = pkg._lib.SUMS_FLOAT, pkg._lib.SUMS_UNIT
    for e in (pkg.sums_exponent(m), -12):
        sums, f = packed.label_sums(lab, 6, e, FLOAT)
        assert np.array_equal(bits(f), bits(pkg.close_sums(sums, e, FLOAT)))
        assert np.allclose(f.astype(np.float64), sums.astype(np.float64) * 2.0 ** e, rtol=2.0 ** -24, atol=0)  # one rounding to fp32
        prev = np.full((6, m.cols), -7.0, dtype=np.float32)
        sums_u, u = packed.label_sums(lab, 6, e, UNIT, out=prev)
        assert np.array_equal(sums_u, sums)
        assert np.array_equal(bits(u), bits(pkg.close_sums(sums, e, UNIT, out=prev)))
        assert np.all(u[3] == -7.0) and not np.any(u[[0, 1, 2, 4, 5]] == -7.0), "an empty bin is left untouched, the others are written"
        norms = np.sqrt((u[[0, 1, 2, 4, 5]].astype(np.float64) ** 2).sum(axis=1))
        assert np.all(np.abs(norms - 1.0) < 1e-6), norms
        # the closing rule alone, over sums the caller holds
        out = prev.copy()
        assert pkg._lib.lib().tkspmv_sums_close_host(sums.ctypes.data_as(I64P), 6, m.cols, e, UNIT, out.ctypes.data_as(F32P)) == 0
        assert np.array_equal(bits(out), bits(u))
    # a zero sum and an overflowed norm are not written either
    s = np.zeros((3, 70), dtype=np.int64)
    s[1, :] = 1 << 40
    s[2, 5] = 3
    got = pkg.close_sums(s, 60, UNIT, out=np.full((3, 70), 9.0, dtype=np.float32))  # bin 1: 70 * 2^200 overflows fp32
    assert np.all(got[0] == 9.0) and np.all(got[1] == 9.0) and got[2, 5] == 1.0 and np.all(np.delete(got[2], 5) == 0.0)
    out = np.full((3, 70), 9.0, dtype=np.float32)
    assert pkg._lib.lib().tkspmv_sums_close_host(s.ctypes.data_as(I64P), 3, 70, 60, UNIT, out.ctypes.data_as(F32P)) == 0
    assert np.array_equal(bits(out), bits(got))


def test_default_exponent(pkg):
    """Packed.sums_exponent == host.sums_exponent on every matrix, and with it no word can reach 2^63 even with ONE bin (the
    worst case: every entry of a column in the same word), also where every entry of the fullest column is the largest value."""
    worst = coo(pkg, 1000, 16, np.arange(1000), np.full(1000, 5), np.full(1000, np.nextafter(np.float32(2), np.float32(1))))
    for name, m in list(_matrices(pkg)) + [("worst", worst), ("one", coo(pkg, 3, 4, [1], [2], [-0.375]))]:
        e = pkg.sums_exponent(m)
        for packed, label in _packings(pkg, m, hints=(7,)):
            assert packed.sums_exponent() == e, (name, label)
            sums, _ = packed.label_sums(np.zeros(m.rows, dtype=np.uint32), 1, e)
            assert np.max(np.abs(sums.astype(np.float64))) < 2.0 ** 63, name  # (the issue's 2^62 * 2)
            assert np.array_equal(sums, pkg.label_sums(m, np.zeros(m.rows, dtype=np.uint32), 1, e)), name
    assert np.max(np.abs(pkg.label_sums(worst, np.zeros(1000, dtype=np.uint32), 1, pkg.sums_exponent(worst)))) > 2 ** 61, "the worst case is not near the bound"
    assert pkg.sums_exponent(coo(pkg, 5, 4, [], [], [])) == 0
    assert pkg.Packed(coo(pkg, 5, 4, [], [], []), k=2).sums_exponent() == 0
    assert pkg.sums_exponent(coo(pkg, 3, 4, [1], [2], [-0.375])) == -2 + 1 + 0 - 62


def test_sums_against_float64_column_sums(pkg):
    """Independent of the grid: |ldexp(sums, E) - the column sums of the COO| <= n_bc 2^(E-1) per word, n_bc the entries of the bin
    and column -- half a quantum per rounded value, the bound of the rounding rule. The float64 sums of the reference are themselves
    off by at most n 2^-53 times the sum of the magnitudes, and float64(sums) by 2^-53 relative: that error, not the code's, is the
    added term abs_sum 2^-45."""
    m = _wide(pkg, pkg.generate_matrix(2500, 1024, 20, "gamma", 4), 4)
    n_bins = 5
    lab = _labels(m.rows, n_bins, 2)
    keep = lab[m.row] < n_bins
    key = lab[m.row][keep].astype(np.int64) * m.cols + m.col[keep]
    exact = np.zeros(n_bins * m.cols)
    mag = np.zeros(n_bins * m.cols)
    np.add.at(exact, key, m.val[keep].astype(np.float64))
    np.add.at(mag, key, np.abs(m.val[keep]).astype(np.float64))
    n_bc = np.bincount(key, minlength=n_bins * m.cols).astype(np.float64)
    packed = pkg.Packed(m, k=8, n_wave_partitions=32)
    for e in (pkg.sums_exponent(m), -30, -12, -3):
        sums, _ = packed.label_sums(lab, n_bins, e)
        err = np.abs(sums.ravel().astype(np.float64) * 2.0 ** e - exact)
        assert np.all(err <= n_bc * 2.0 ** (e - 1) + mag * 2.0 ** -45), (e, float(err.max()))


def test_assign_and_label_sums_chain_is_spherical_kmeans(pkg):
    """Three iterations of Packed.assign + Packed.label_sums(UNIT, out = the centroids): as bits against the restatements
    (host.label_sums + host.close_sums on the twin's labels), and against the k-means recipe in float64 -- np.add.at over the COO,
    normalised, an empty cluster keeping its vector -- within what one fp32 rounding per value and per product allows."""
    m = signed(pkg, pkg.generate_matrix(1500, 300, 12, "gamma", 6), 6)
    packed = pkg.Packed(m, k=8, n_wave_partitions=16)
    e = packed.sums_exponent()
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((6, 300)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    cent[5] = cent[2]  # (ties go to the smaller index: the duplicate never wins a row, its cluster ends empty)
    was_empty = False
    for _ in range(3):
        labels, _ = packed.assign(cent)
        sums, new = packed.label_sums(labels, 6, e, pkg._lib.SUMS_UNIT, out=cent)
        assert np.array_equal(sums, pkg.label_sums(m, labels, 6, e))
        assert np.array_equal(bits(new), bits(pkg.close_sums(sums, e, pkg._lib.SUMS_UNIT, out=cent)))
        ref = np.zeros((6, 300))
        np.add.at(ref, (labels[m.row].astype(np.int64), m.col.astype(np.int64)), m.val.astype(np.float64))
        for b in range(6):
            nrm = np.linalg.norm(ref[b])
            if nrm == 0:
                was_empty = True
                assert np.array_equal(bits(new[b]), bits(cent[b])), "an empty cluster keeps its vector"
            else:
                assert np.allclose(new[b], ref[b] / nrm, rtol=0, atol=1e-6), b
        cent = new
    assert was_empty, "no cluster ever ended empty: the keep rule was not exercised"


def test_argument_checks(pkg):
    lib = pkg._lib.lib()
    INVALID, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    lab = np.zeros(m.rows, dtype=np.uint32)
    sums = np.full((2, 64), -7, dtype=np.int64)
    out = np.full((2, 64), -7.0, dtype=np.float32)
    Lb, S, O = lab.ctypes.data_as(U32P), sums.ctypes.data_as(I64P), out.ctypes.data_as(F32P)
    e = C.c_int32(77)
    # a NULL engine: INVALID from every entry point (no engine, hence no device, is ever touched)
    assert lib.tkspmv_enqueue_label_sums(None, C.c_void_p(64), 2, 0, 0, C.c_void_p(64), 0, None, None) == INVALID
    assert lib.tkspmv_enqueue_sums_close(None, C.c_void_p(64), 2, 0, 1, C.c_void_p(64), None) == INVALID
    assert lib.tkspmv_sums_exponent(None, C.byref(e)) == INVALID and e.value == 77
    assert lib.tkspmv_label_sums(None, Lb, 2, 0, 0, S, None) == INVALID
    packed = pkg.Packed(m, k=8)
    assert lib.tkspmv_packed_label_sums(None, Lb, 2, 0, 0, S, None) == INVALID
    assert lib.tkspmv_packed_label_sums(packed._h, None, 2, 0, 0, S, None) == INVALID
    assert lib.tkspmv_packed_label_sums(packed._h, Lb, 0, 0, 0, S, None) == INVALID
    assert lib.tkspmv_packed_label_sums(packed._h, Lb, 2, 0, 3, S, O) == INVALID and lib.tkspmv_packed_label_sums(packed._h, Lb, 2, 0, -1, S, O) == INVALID
    assert lib.tkspmv_packed_label_sums(packed._h, Lb, 2, 0, 1, S, None) == INVALID and lib.tkspmv_packed_label_sums(packed._h, Lb, 2, 0, 2, S, None) == INVALID
    assert lib.tkspmv_packed_sums_exponent(None, C.byref(e)) == INVALID and lib.tkspmv_packed_sums_exponent(packed._h, None) == INVALID
    assert lib.tkspmv_sums_close_host(None, 2, 64, 0, 1, O) == INVALID and lib.tkspmv_sums_close_host(S, 2, 64, 0, 0, O) == INVALID
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        p = pkg.Packed(m, k=8, precision=prec)
        assert lib.tkspmv_packed_label_sums(p._h, Lb, 2, 0, 1, S, O) == UNSUPPORTED, prec
        assert lib.tkspmv_packed_sums_exponent(p._h, C.byref(e)) == UNSUPPORTED, prec
        with pytest.raises(pkg.TkspmvError) as err:
            p.label_sums(lab, 2, 0)
        assert err.value.status == UNSUPPORTED
        p.close()
    assert np.all(sums == -7) and np.all(out == -7.0) and e.value == 77, "a rejected call wrote its output"
    assert lib.tkspmv_packed_label_sums(packed._h, Lb, 2, -20, 1, None, O) == 0 and np.all(sums == -7) and not np.any(out == -7.0)  # sums may be NULL
    assert lib.tkspmv_packed_label_sums(packed._h, Lb, 2, -20, 0, S, None) == 0 and np.all(sums[1] == 0) and np.any(sums[0] != 0)
    with pytest.raises(ValueError):
        packed.label_sums(lab[:-1], 2, 0)
    with pytest.raises(ValueError):
        pkg.label_sums(m, lab[:-1], 2, 0)
