"""Boosted range, facet and grouped queries without a GPU: the symbols of every layer, argument checks that come before any device
call, and the numpy restatement of the range contract (boosted_matches) pinned to a plain loop over float32 scalars."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approximate-spmv-topk_amd", "csrc")
FORMS = ("range", "facets", "grouped")
NAMES = tuple(f"tkspmv_{kind}_boosted_{form}" for form in FORMS for kind in ("enqueue", "run"))
NINF = np.float32(-np.inf)


def _f32(a):
    return np.array(a, dtype=np.float32)


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    capi = open(os.path.join(CSRC, "c_api.cpp")).read()
    lib = pkg._lib.lib()
    for name in NAMES:
        assert name in pkg._lib.EXPORTED_SYMBOLS
        assert f"int {name}(" in hdr and f"int {name}(" in capi
        assert hasattr(lib, name)
    for form in FORMS:
        assert callable(getattr(pkg.SpMV, f"enqueue_boosted_{form}")) and callable(getattr(pkg.SpMV, f"run_boosted_{form}"))
    for name in ("boosted_range_spmv", "boosted_facet_spmv", "boosted_grouped_spmv", "cosine_range_spmv", "boosted_matches"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert '#include "kernels/boost_forms.hpp"' in open(os.path.join(CSRC, "engine.hip")).read()
    assert "Not available in range, facet and grouped queries" not in hdr


def test_null_engine_fails_before_any_device_call(pkg):
    L, lib = pkg._lib, pkg._lib.lib()
    count, n = C.c_uint64(7), C.c_int32(9)
    assert lib.tkspmv_enqueue_boosted_range(None, None, 1, None, None, 0, None, None, 0, None, None, 0, None, None) == L.ERR_INVALID
    assert lib.tkspmv_run_boosted_range(None, 0.5, 0, None, None, 0, C.byref(count)) == L.ERR_INVALID
    assert lib.tkspmv_enqueue_boosted_facets(None, None, 1, None, None, 0, None, None, 0, None, 0, None, None, None, None) == L.ERR_INVALID
    assert lib.tkspmv_run_boosted_facets(None, 0.5, 0, None, None, C.byref(count)) == L.ERR_INVALID
    assert lib.tkspmv_enqueue_boosted_grouped(None, None, 1, None, None, 0, None, 0, None, None, None, None, None) == L.ERR_INVALID
    assert lib.tkspmv_run_boosted_grouped(None, 0, None, None, None, C.byref(n)) == L.ERR_INVALID
    assert count.value == 7 and n.value == 9


def _loop(y, present, tau, w, b, allow, first_row):
    """The contract as a plain loop over float32 scalars; the matches sorted by (score descending, row descending)."""
    tau = np.float32(tau)
    hits = []
    with np.errstate(all="ignore"):
        for r in range(len(y)):
            if not present[r] or (allow is not None and not allow[r]):
                continue
            s = np.float32(y[r])
            if s == NINF:
                continue
            t = np.float32(np.float32(w[r]) * s) if w is not None else s
            t = np.float32(t + np.float32(b[r])) if b is not None else t
            if not np.isfinite(t):
                continue
            if t >= tau:
                hits.append((float(t), r + first_row, t))
    hits.sort(key=lambda h: (h[0], h[1]), reverse=True)
    return np.array([h[1] for h in hits], dtype=np.uint32), np.array([h[2] for h in hits], dtype=np.float32), len(hits)


def _same(got, want, what):
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (what, "rows")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "score bits")


#          0    1     2      3    4            5    6     7     8    9    10    11         12           13
Y = _f32([0.0, -0.0, -np.inf, 2.0, 2.0 ** -100, 1.5, -2.5, -0.0, 0.0, 3.0, -0.0, 1.0000001, 2.0 ** -126, 0.75])
W = _f32([1.0, 1.0, 0.0, 3e38, 2.0 ** -40, 0.0, -1.0, -2.0, -2.0, 0.3333333, 0.0, 1.0000001, 0.5, 1.0])
B = _f32([-0.0, 0.0, 5.0, 0.0, -0.0, 0.25, 1.0, -0.0, 0.0, 1e-8, -0.0, -1.0, 2.0 ** -149, np.nan])


def test_boosted_matches_is_the_loop_on_special_values(pkg):
    present = np.ones(Y.size, dtype=bool)
    present[9] = False
    allow = np.ones(Y.size, dtype=bool)
    allow[5] = False
    sb = pkg.boost_scores(Y, W, B)
    assert sb[3] == NINF and sb[13] == NINF and sb[2] == NINF  # an overflowing product, a NaN sum, a row that holds -inf
    assert sb[4] == np.float32(2.0 ** -140) != 0                # a subnormal product
    taus = [-np.inf, np.nan, np.inf, 0.0, -0.0, 2.0 ** -140, float(sb[6]), float(sb[12]), float(np.nextafter(sb[6], np.float32(np.inf))), -1e30]
    for tau in taus:
        for ww, bb in ((W, None), (None, B), (W, B)):
            for al in (None, allow):
                for first_row in (0, 1000):
                    got = pkg.boosted_matches(Y, present, tau, ww, bb, al, first_row)
                    _same(got, _loop(Y, present, tau, ww, bb, al, first_row), (tau, ww is not None, bb is not None, al is not None, first_row))
    idx, val, n = pkg.boosted_matches(Y, present, -np.inf, W, B)
    assert n == Y.size - 4 and not set(idx.tolist()) & {2, 3, 9, 13}  # -inf: every present row with a finite s', the excluded ones never
    assert pkg.boosted_matches(Y, present, np.nan, W, B)[2] == 0        # NaN: nothing
    assert 4 in pkg.boosted_matches(Y, present, 2.0 ** -140, W, B)[0]   # a threshold that is exactly a row's s' (a subnormal) keeps the row
    assert 4 not in pkg.boosted_matches(Y, present, 2.0 ** -139, W, B)[0]
    idx, val, n = pkg.boosted_matches(Y, present, 3.5, W, B)            # exactly row 6's s' (w < 0)
    assert idx.tolist() == [6] and val[0] == 3.5
    idx, val, n = pkg.boosted_matches(Y, present, 0.25, W, B)           # w = 0: the bias alone, exactly at the threshold
    assert 5 in idx and val[idx.tolist().index(5)].view(np.uint32) == _f32([0.25]).view(np.uint32)[0]
    both = pkg.boosted_matches(Y, present, 0.0, W, B)                    # +-0 compare equal to the threshold 0.0: both kinds match
    zeros = both[1][both[1] == 0]
    assert set(zeros.view(np.uint32).tolist()) == {0, 0x80000000}
    with pytest.raises(ValueError):
        pkg.boosted_matches(Y, present[:-1], 0.0)
    with pytest.raises(ValueError):
        pkg.boosted_matches(Y, present, 0.0, allow=allow.astype(np.uint8))


def test_identities_on_bits_against_a_plain_threshold(pkg):
    rng = np.random.default_rng(3)
    y = np.concatenate([rng.standard_normal(500).astype(np.float32), _f32([0.0, -0.0, -np.inf, 2.0 ** -140, -2.0 ** -130, 3e38, -3e38])])
    present = rng.random(y.size) < 0.9
    present[500:] = True
    ones, nz = np.ones_like(y), np.full_like(y, -0.0)
    for tau in (-np.inf, -0.5, 0.0, -0.0, float(y[17]), 2.0 ** -140, 1e38, np.nan, np.inf):
        with np.errstate(invalid="ignore"):
            rows = np.flatnonzero(present & (y > -np.inf) & (y >= np.float32(tau)))
        rows = rows[np.lexsort((rows, y[rows]))[::-1]]
        want = (rows.astype(np.uint32), y[rows], int(rows.size))
        _same(pkg.boosted_matches(y, present, tau, ones), want, ("w = 1", tau))
        _same(pkg.boosted_matches(y, present, tau, None, nz), want, ("b = -0.0", tau))
        _same(pkg.boosted_matches(y, present, tau), want, ("no boost", tau))
