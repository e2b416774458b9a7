"""Facet counts without a GPU: the symbols of every layer, the FACET_LDS_BINS option, facet_counts (the contract restated in numpy)
against a plain Python loop, and the argument check that comes before any device call and needs no engine."""
import ctypes as C
import math
import os
import struct

import numpy as np

from support import bits_of, order_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facet_symbols_in_every_layer(pkg):
    assert "tkspmv_enqueue_facets" in pkg._lib.EXPORTED_SYMBOLS and "tkspmv_run_facets" in pkg._lib.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    assert "int tkspmv_enqueue_facets(" in hdr and "int tkspmv_run_facets(" in hdr and "tkspmv_facet_best;" in hdr
    lib = pkg._lib.lib()
    assert hasattr(lib, "tkspmv_enqueue_facets") and hasattr(lib, "tkspmv_run_facets")
    assert C.sizeof(pkg._lib.FacetBest) == 8 and [n for n, _ in pkg._lib.FacetBest._fields_] == ["row", "score_bits"]
    for name in ("enqueue_facets", "run_facets"):
        assert callable(getattr(pkg.SpMV, name))
    assert callable(pkg.facet_spmv) and "facet_spmv" in pkg.__all__
    assert callable(pkg.facet_counts) and "facet_counts" in pkg.__all__


def test_facet_lds_bins_is_a_documented_option(pkg):
    opts = {o["name"]: o for o in pkg.options()}
    assert "FACET_LDS_BINS" in opts
    assert opts["FACET_LDS_BINS"]["kind"] == "tuning" and opts["FACET_LDS_BINS"]["doc"] and opts["FACET_LDS_BINS"]["values"]
    pkg.set_option("FACET_LDS_BINS", 0)
    assert pkg.get_option("FACET_LDS_BINS") == "0"
    pkg.set_option("FACET_LDS_BINS", 64)
    assert pkg.get_option("FACET_LDS_BINS") == "64"
    pkg.set_option("FACET_LDS_BINS", None)
    assert pkg.get_option("FACET_LDS_BINS") is None


def test_null_engine_fails_before_any_device_call(pkg):
    """The one argument error the library can report without an engine; the others need one and are in test_gpu_facets.py."""
    lib = pkg._lib.lib()
    total = C.c_uint64(7)
    counts = (C.c_uint32 * 2)(5, 5)
    assert lib.tkspmv_enqueue_facets(None, None, 1, None, None, 0, None, 0, None, None, None, None) == pkg._lib.ERR_INVALID
    assert lib.tkspmv_run_facets(None, 0.5, 0, counts, None, C.byref(total)) == pkg._lib.ERR_INVALID
    assert total.value == 7 and list(counts) == [5, 5]


def _loop(scores, present, labels, n_bins, threshold, first_row=0, allow=None):
    """The contract, row by row in plain Python: fp32 >=, the best by (order key << 32 | global row)."""
    counts, best, total = [0] * n_bins, [0] * n_bins, 0
    t = struct.unpack("<f", struct.pack("<f", threshold))[0]
    for r, s in enumerate(scores):
        s = float(s)
        if not present[r] or (allow is not None and not allow[r]) or math.isnan(s) or math.isnan(t) or not s >= t:
            continue
        total += 1
        b = int(labels[r])
        if b >= n_bins:
            continue
        counts[b] += 1
        best[b] = max(best[b], (order_key(s) << 32) | (first_row + r))
    bi = [k & 0xFFFFFFFF if c else 0 for k, c in zip(best, counts)]
    bv = []
    for k, c in zip(best, counts):
        hi = k >> 32
        bv.append(((hi & 0x7FFFFFFF) if hi & 0x80000000 else (~hi & 0xFFFFFFFF)) if c else 0)
    return counts, bi, bv, total


def _same(pkg, scores, present, labels, n_bins, threshold, **kw):
    scores = np.asarray(scores, dtype=np.float32)
    counts, bi, bv, total = pkg.facet_counts(scores, present, labels, n_bins, threshold, **kw)
    assert counts.dtype == np.uint32 and bi.dtype == np.uint32 and bv.dtype == np.float32
    assert counts.shape == bi.shape == bv.shape == (n_bins,)
    ec, ei, ev, et = _loop(scores, present, labels, n_bins, threshold, **kw)
    assert counts.tolist() == ec and bi.tolist() == ei and bv.view(np.uint32).tolist() == ev and total == et
    # every match is in a bin or has a label beyond the bins
    ok = np.asarray(present, dtype=bool) & (True if kw.get("allow") is None else np.asarray(kw["allow"]))
    with np.errstate(invalid="ignore"):
        ok = ok & (scores >= np.float32(threshold))
    assert int(counts.sum()) + int(np.count_nonzero(ok & (np.asarray(labels).astype(np.int64) >= n_bins))) == total
    return counts, bi, bv, total


def test_facet_counts_small_cases(pkg):
    NF = 0xFFFFFFFF
    ones = np.ones(8, dtype=bool)
    # ties for a bin's best: the larger row id wins
    c, bi, bv, t = _same(pkg, [0.5, 0.5, 0.25, 0.5, 0.1, 0.5, 0.7, 0.7], ones, [0, 0, 0, 1, 1, 1, 2, 2], 3, 0.2)
    assert c.tolist() == [3, 2, 2] and bi.tolist() == [1, 5, 7] and bv.tolist() == [0.5, 0.5, np.float32(0.7)] and t == 7
    # -0.0 against +0.0: equal as floats (both match a threshold of 0.0 and of -0.0), +0.0 ranks first whatever the row ids
    for thr in (0.0, -0.0):
        c, bi, bv, t = _same(pkg, [0.0, -0.0, -0.0, 0.0, -0.0, -1.0, -0.0, -0.0], ones, [0, 0, 1, 1, 2, 2, 2, 3], 4, thr)
        assert c.tolist() == [2, 2, 2, 1] and bi.tolist() == [0, 3, 6, 7] and t == 7
        assert bv.view(np.uint32).tolist() == [0, 0, 0x80000000, 0x80000000]
    # labels >= n_bins belong to no bin and count in the total; an empty bin gives (0, 0.0)
    c, bi, bv, t = _same(pkg, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2], ones, [0, NF, 5, 3, 0, NF, 2, 0], 3, 0.25)
    assert c.tolist() == [2, 0, 1] and bi.tolist() == [0, 0, 6] and bv.view(np.uint32).tolist() == [bits_of(np.float32(0.9)), 0, bits_of(np.float32(0.3))] and t == 7
    # -inf matches every present row (also one that scores -inf), NaN nothing; a NaN score never matches
    present = np.array([1, 1, 0, 1, 1, 1, 0, 1], dtype=bool)
    sc = [0.1, -np.inf, 0.9, np.nan, -3.0, 2.0, 0.2, 0.0]
    c, bi, bv, t = _same(pkg, sc, present, [0, 1, 0, 0, 1, 1, 0, 0], 2, -np.inf)
    assert c.tolist() == [2, 3] and t == 5 and bi.tolist() == [0, 5]
    c, bi, bv, t = _same(pkg, sc, present, [0, 1, 0, 0, 1, 1, 0, 0], 2, np.nan)
    assert c.tolist() == [0, 0] and t == 0 and bi.tolist() == [0, 0] and bv.view(np.uint32).tolist() == [0, 0]
    # first_row: global ids in best_idx, also for a tie
    c, bi, bv, t = _same(pkg, [0.5, 0.5, 0.1, 0.9], np.ones(4, dtype=bool), [0, 0, 1, 1], 2, 0.0, first_row=5000)
    assert bi.tolist() == [5001, 5003]
    # an allow mask
    allow = np.array([0, 1, 1, 0, 1, 1, 1, 0], dtype=bool)
    c, bi, bv, t = _same(pkg, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2], ones, [0, 0, 1, 1, 2, 2, 0, 1], 3, 0.35, allow=allow)
    assert c.tolist() == [1, 1, 2] and bi.tolist() == [1, 2, 4] and t == 4


def test_facet_counts_random(pkg):
    rng = np.random.default_rng(5)
    for n_bins in (1, 7, 300):
        rows = 400
        scores = rng.choice(np.float32([-1.0, -0.0, 0.0, 0.25, 0.5, 0.75, 1.5]), rows)  # many ties
        present = rng.random(rows) < 0.9
        labels = rng.integers(0, n_bins + 2, rows).astype(np.uint32)
        labels[rng.random(rows) < 0.05] = 0xFFFFFFFF
        allow = rng.random(rows) < 0.7
        for thr in (-np.inf, -0.5, 0.0, 0.5, 2.0, np.nan):
            _same(pkg, scores, present, labels, n_bins, thr, first_row=123, allow=allow)
            _same(pkg, scores, present, labels, n_bins, thr)
