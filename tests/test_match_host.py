"""Term predicates without a GPU: the symbols of every layer, bool_query's bit assignment and errors, match_rows (the contract
restated in numpy) on a hand-written COO and against a plain Python loop, the record's size, and the argument check that comes before
any device call and needs no engine."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_symbols_in_every_layer(pkg):
    assert "tkspmv_enqueue_match" in pkg._lib.EXPORTED_SYMBOLS and "tkspmv_run_match" in pkg._lib.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    assert "int tkspmv_enqueue_match(" in hdr and "int tkspmv_run_match(" in hdr and "tkspmv_match;" in hdr
    lib = pkg._lib.lib()
    assert hasattr(lib, "tkspmv_enqueue_match") and hasattr(lib, "tkspmv_run_match")
    assert [n for n, _ in pkg._lib.Match._fields_] == ["must", "must_not", "should", "min_should"]
    for name in ("enqueue_match", "match"):
        assert callable(getattr(pkg.SpMV, name))
    for name in ("bool_query", "match_rows"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__


def test_record_is_16_bytes(pkg):
    src = '#include <stdio.h>\n#include "tkspmv.h"\nint main(void) { printf("%zu\\n", sizeof(tkspmv_match)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert int(out[0]) == 16 == C.sizeof(pkg._lib.Match)


def test_null_arguments_fail_before_any_device_call(pkg):
    """The argument error the library can report without an engine; the others need one and are in test_gpu_match.py."""
    lib = pkg._lib.lib()
    count = C.c_uint64(7)
    words = (C.c_uint32 * 2)(5, 5)
    table = (C.c_uint32 * 4)(1, 1, 1, 1)
    pred = pkg._lib.Match(1, 0, 0, 0)
    assert lib.tkspmv_enqueue_match(None, None, 0, None, 1, None, 0, None, 0, None, None) == pkg._lib.ERR_INVALID
    assert lib.tkspmv_run_match(None, table, C.byref(pred), 0, 0, words, C.byref(count)) == pkg._lib.ERR_INVALID
    assert count.value == 7 and list(words) == [5, 5]
    assert b"NULL engine" in lib.tkspmv_last_error()


def test_bool_query_bits(pkg):
    t, pred = pkg.bool_query(1024)
    assert t.dtype == np.uint32 and t.shape == (1024,) and not t.any() and pred == (0, 0, 0, 0)
    # must first, then should, then one bit for all of must_not; an item is a column or an iterable of columns
    t, (must, must_not, should, min_should) = pkg.bool_query(1024, must=[17, (40, 41)], must_not=[900, [901, 17]], should=[5, range(6, 9), np.array([9])], min_should=2)
    assert (must, should, must_not, min_should) == (0b11, 0b11100, 0b100000, 2)
    exp = np.zeros(1024, dtype=np.uint32)
    exp[17] = 1 | 32
    exp[[40, 41]] = 2
    exp[5] = 4
    exp[[6, 7, 8]] = 8
    exp[9] = 16
    exp[[900, 901]] = 32
    assert np.array_equal(t, exp)
    # 32 clauses fit, the last one is bit 31; a 33rd does not
    t, pred = pkg.bool_query(64, must=list(range(31)), must_not=[63])
    assert pred == (0x7FFFFFFF, 0x80000000, 0, 0) and t[63] == 0x80000000 and t[30] == 1 << 30
    t, pred = pkg.bool_query(64, should=list(range(32)), min_should=40)
    assert pred == (0, 0, 0xFFFFFFFF, 40)
    with pytest.raises(ValueError):
        pkg.bool_query(64, must=list(range(32)), must_not=[63])
    with pytest.raises(ValueError):
        pkg.bool_query(64, must=list(range(20)), should=list(range(13)))
    for bad in (dict(must=[64]), dict(must=[-1]), dict(should=[(3, 64)]), dict(must_not=[1024])):
        with pytest.raises(ValueError):
            pkg.bool_query(64, **bad)


# 12 rows x 16 columns. Row 2 is empty; row 3 repeats column 5; row 4's only entry (column 7) is an explicit zero.
COO = [(0, 1), (0, 2), (1, 2), (3, 5), (3, 5), (3, 1), (4, 7), (5, 1), (5, 2), (5, 5), (6, 9), (7, 15), (7, 1), (8, 2), (8, 9),
       (9, 5), (10, 7), (10, 9), (11, 15)]
ROW = np.array([r for r, _ in COO], dtype=np.uint32)
COL = np.array([c for _, c in COO], dtype=np.uint32)


def _rows(pkg, allow=None, **q):
    t, pred = pkg.bool_query(16, **q)
    got = pkg.match_rows(ROW, COL, 12, t, pred, allow=allow)
    assert got.dtype == np.bool_ and got.shape == (12,)
    # ... and the contract row by row in plain Python
    sets = {r: set() for r in range(12)}
    for r, c in COO:
        sets[r].add(c)
    items = lambda x: set(x) if hasattr(x, "__iter__") else {x}
    exp = []
    for r in range(12):
        s = sets[r]
        ok = bool(s) and all(s & items(m) for m in q.get("must", ())) and not any(s & items(m) for m in q.get("must_not", ()))
        ok = ok and sum(1 for m in q.get("should", ()) if s & items(m)) >= q.get("min_should", 0)
        exp.append(ok and (allow is None or bool(allow[r])))
    assert got.tolist() == exp, (q, got.tolist(), exp)
    return np.flatnonzero(got).tolist()


def test_match_rows_hand_written(pkg):
    assert _rows(pkg) == [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]                      # all-zero fields: every row with entries, not the empty row 2
    assert _rows(pkg, must=[5]) == [3, 5, 9]                                       # a repeated column changes nothing
    assert _rows(pkg, must=[7]) == [4, 10]                                         # an explicit zero is an entry
    assert _rows(pkg, must=[1, 2]) == [0, 5]
    assert _rows(pkg, must=[(1, 9)], must_not=[2]) == [3, 6, 7, 10]
    assert _rows(pkg, must_not=[1, 9]) == [1, 4, 9, 11]                            # must_not only; the empty row stays out
    sh = [1, 2, 5]
    assert _rows(pkg, should=sh, min_should=0) == [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    assert _rows(pkg, should=sh, min_should=1) == [0, 1, 3, 5, 7, 8, 9]
    assert _rows(pkg, should=sh, min_should=2) == [0, 3, 5]
    assert _rows(pkg, should=sh, min_should=3) == [5]
    assert _rows(pkg, should=sh, min_should=4) == []                               # more than the clauses there are: nothing
    allow = np.zeros(12, dtype=bool)
    allow[[2, 3, 4, 9]] = True
    assert _rows(pkg, allow=allow, must=[5]) == [3, 9]
    assert _rows(pkg, allow=allow) == [3, 4, 9]
    # clause bit 31 on its own, and a column that belongs to all 32 clauses
    t = np.zeros(16, dtype=np.uint32)
    t[15] = 0x80000000
    assert np.flatnonzero(pkg.match_rows(ROW, COL, 12, t, (0x80000000, 0, 0, 0))).tolist() == [7, 11]
    assert np.flatnonzero(pkg.match_rows(ROW, COL, 12, t, (0, 0x80000000, 0, 0))).tolist() == [0, 1, 3, 4, 5, 6, 8, 9, 10]
    t[:] = 0
    t[9] = 0xFFFFFFFF
    assert np.flatnonzero(pkg.match_rows(ROW, COL, 12, t, (0xFFFFFFFF, 0, 0xFFFFFFFF, 32))).tolist() == [6, 8, 10]
    assert np.flatnonzero(pkg.match_rows(ROW, COL, 12, t, (0, 0, 0xFFFFFFFF, 33))).tolist() == []
    with pytest.raises(ValueError):
        pkg.match_rows(ROW, COL, 11, t, (0, 0, 0, 0))
    with pytest.raises(ValueError):
        pkg.match_rows(ROW, COL, 12, t[:15], (0, 0, 0, 0))
    with pytest.raises(ValueError):
        pkg.match_rows(ROW, COL, 12, t, (0, 0, 0, 0), allow=np.ones(11, dtype=bool))


def test_match_rows_packs_like_row_mask(pkg):
    """The expectation of the GPU tests: match_rows packed with row_mask, tail bits 0, popcount = the count."""
    t, pred = pkg.bool_query(16, must=[5])
    words = pkg.row_mask(12, pkg.match_rows(ROW, COL, 12, t, pred))
    assert words.tolist() == [(1 << 3) | (1 << 5) | (1 << 9)]
