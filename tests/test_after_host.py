"""Search-after paging without a GPU: the symbols of every layer, the cursor's size on both sides, argument checks that come before
any device call, the numpy restatement of the contract (page_after) pinned to the oracle's selection and to a plain loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from support import bits_of, order_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approximate-spmv-topk_amd", "csrc")
NAMES = ("tkspmv_enqueue_after", "tkspmv_run_after")
START, AFTER, END = 0, 1, 2


def test_after_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    capi = open(os.path.join(CSRC, "c_api.cpp")).read()
    lib = pkg._lib.lib()
    for name in NAMES:
        assert name in pkg._lib.EXPORTED_SYMBOLS
        assert f"int {name}(" in hdr and f"int {name}(" in capi
        assert hasattr(lib, name)
    assert "tkspmv_cursor" in hdr and "12 bytes per row" in hdr
    for name in ("enqueue_after", "run_after", "pages"):
        assert callable(getattr(pkg.SpMV, name))
    assert callable(pkg.ranked_spmv) and "ranked_spmv" in pkg.__all__
    assert callable(pkg.page_after) and "page_after" in pkg.__all__
    assert (pkg.CURSOR_START, pkg.CURSOR_AFTER, pkg.CURSOR_END) == (START, AFTER, END)


def test_cursor_is_sixteen_bytes_on_both_sides(pkg, tmp_path):
    assert C.sizeof(pkg._lib.Cursor) == 16
    assert [f[0] for f in pkg._lib.Cursor._fields_] == ["row", "score_bits", "state", "reserved"]
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} tkspmv_cursor;", hdr)
    assert m, "tkspmv_cursor is not declared as one typedef"
    fields = [f.split() for f in m.group(1).split(";") if f.strip()]
    assert fields == [["uint32_t", "row"], ["uint32_t", "score_bits"], ["uint32_t", "state"], ["uint32_t", "reserved"]]  # four words, no padding
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    assert "sizeof(tkspmv_cursor) == 16" in engine  # the device side's static_assert


def test_null_engine_fails_before_any_device_call(pkg):
    lib = pkg._lib.lib()
    n, total = C.c_int32(7), C.c_uint32(9)
    nxt = pkg._lib.Cursor(11, 12, 13, 14)
    assert lib.tkspmv_enqueue_after(None, None, 1, None, None, 0, None, None, None, None, None, None) == pkg._lib.ERR_INVALID
    assert lib.tkspmv_run_after(None, None, 0, None, None, C.byref(n), C.byref(total), C.byref(nxt)) == pkg._lib.ERR_INVALID
    assert n.value == 7 and total.value == 9 and (nxt.row, nxt.score_bits, nxt.state, nxt.reserved) == (11, 12, 13, 14)


def _loop(y, present, k, cursor, min_score, first_row):
    """The contract as a plain loop: every eligible row behind the cursor by its key, descending; the first k; what is left."""
    kmin = order_key(min_score)
    keyed = [(order_key(y[r]) << 32) | (r + first_row) for r in range(len(y)) if present[r] and order_key(y[r]) >= kmin and y[r] > -np.inf]
    if cursor is not None and cursor[2] == AFTER:
        ceiling = (order_key(np.array([cursor[1]], dtype=np.uint32).view(np.float32)[0]) << 32) | cursor[0]
        keyed = [c for c in keyed if c < ceiling]
    elif cursor is not None and cursor[2] != START:
        keyed = []
    keyed.sort(reverse=True)
    page = [c & 0xFFFFFFFF for c in keyed[:k]]
    nxt = (page[-1], bits_of(y[page[-1] - first_row]), AFTER) if len(keyed) > k else (0, 0, END)
    return page, len(keyed), nxt


def _check(pkg, y, present, k, cursor, min_score=0.0, first_row=0, allow=None):
    idx, val, n, total, nxt = pkg.page_after(y, present, k, cursor, min_score, first_row, allow)
    page, left, want_next = _loop(y, present if allow is None else present & allow, k, cursor, min_score, first_row)
    assert n == len(page) == min(k, left) and total == left
    assert idx[:n].tolist() == page
    assert np.array_equal(val[:n].view(np.uint32), y[np.array(page, dtype=np.int64) - first_row].view(np.uint32))
    assert np.all(idx[n:] == 0) and np.all(val[n:].view(np.uint32) == 0)
    assert nxt == want_next
    return idx, val, n, total, nxt


def test_start_is_the_oracles_selection(pkg, oracle):
    rng = np.random.default_rng(11)
    rows, k = 5003, 100
    y = rng.standard_normal(rows).astype(np.float32)
    present = rng.random(rows) < 0.8
    for min_score, first_row in ((0.0, 0), (float(np.float32(0.4)), 700), (float(np.float32(-0.3)), 0), (2.5, 0)):
        ei, ev = oracle.select_topk(y, present.astype(np.uint8), k, min_score, first_row)
        eligible = int((present & (y >= np.float32(min_score))).sum())
        for cursor in (None, (123, 456, START)):  # (START ignores row and score)
            idx, val, n, total, nxt = pkg.page_after(y, present, k, cursor, min_score, first_row)
            assert np.array_equal(idx, ei) and np.array_equal(val.view(np.uint32), ev.view(np.uint32)), min_score
            assert n == min(k, eligible) and total == eligible
            assert nxt == ((int(ei[k - 1]), int(ev.view(np.uint32)[k - 1]), AFTER) if eligible > k else (0, 0, END))
    assert n < k  # (the last case: fewer than k rows above 2.5 -- the pad of the oracle is the pad of page_after)


@pytest.mark.parametrize("k", [50, 7])
@pytest.mark.parametrize("first_row", [0, 123])
def test_pages_concatenated_are_the_complete_ranking(pkg, oracle, k, first_row):
    rng = np.random.default_rng(5)
    rows = 3001
    y = rng.choice(np.array([-1.0, 0.25, 0.5, 0.5000001, 2.0], dtype=np.float32), rows)  # five values: ties across every page cut
    present = rng.random(rows) < 0.9
    eligible = int((present & (y >= 0)).sum())
    ei, ev = oracle.select_topk(y, present.astype(np.uint8), eligible, 0.0, first_row)
    max_pages = -(-eligible // k)
    got_i, got_v, cursor, pages, left = [], [], None, 0, eligible
    while cursor is None or cursor[2] != END:
        assert pages < max_pages, "the walk must end within ceil(eligible / k) pages"
        idx, val, n, total, cursor = pkg.page_after(y, present, k, cursor, 0.0, first_row)
        assert total == left and n == min(k, left) and n > 0
        got_i.append(idx[:n])
        got_v.append(val[:n])
        left -= n
        pages += 1
    assert pages == max_pages and left == 0
    assert np.array_equal(np.concatenate(got_i), ei) and np.array_equal(np.concatenate(got_v).view(np.uint32), ev.view(np.uint32))


def test_cursors_that_name_no_row_of_the_engine(pkg):
    rng = np.random.default_rng(17)
    rows, k, first_row = 3001, 50, 1000
    values = np.array([-1.0, 0.25, 0.5, 0.5000001, 2.0], dtype=np.float32)
    y = rng.choice(values, rows)
    present = rng.random(rows) < 0.7
    allow = rng.random(rows) < 0.5
    absent = int(np.flatnonzero(~present & (y == 0.5))[0])
    masked = int(np.flatnonzero(present & ~allow & (y == 0.5))[0])
    cursors = [
        (absent + first_row, bits_of(0.5), AFTER),        # a row without entries
        (masked + first_row, bits_of(0.5), AFTER),        # a masked row
        (5, bits_of(0.5), AFTER),                         # below first_row: another shard's row
        (first_row + rows + 77, bits_of(0.5), AFTER),     # above the last row
        (0xFFFFFFFF, bits_of(0.5), AFTER),                # in front of every row with that score
        (0, bits_of(0.5), AFTER),                         # behind every row with that score
        (first_row + 1500, bits_of(0.3), AFTER),          # a score between two values
        (first_row + 1500, bits_of(7.0), AFTER),          # above every score: the whole ranking
        (first_row + 1500, bits_of(-3.0), AFTER),         # below min_score: nothing
        (first_row + 1500, bits_of(0.5), END), (1, 2, 3), (1, 2, 0xFFFFFFFF),  # END, and the states that act as END
    ]
    for cursor in cursors:
        for a in (None, allow):
            _check(pkg, y, present, k, cursor, 0.0, first_row, a)
            _check(pkg, y, present, k, cursor, 0.5, first_row, a)  # min_score on the middle value: ties at the threshold itself
    top = _check(pkg, y, present, k, None, 0.0, first_row, allow)
    assert _check(pkg, y, present, k, cursors[7], 0.0, first_row, allow)[0].tolist() == top[0].tolist()
    assert _check(pkg, y, present, k, cursors[8], 0.0, first_row, allow)[2:] == (0, 0, (0, 0, END))
    assert _check(pkg, y, present, k, cursors[9], 0.0, first_row, allow)[2:] == (0, 0, (0, 0, END))


def test_total_and_next(pkg):
    y = np.arange(1, 21, dtype=np.float32)  # rows 0..19, the best is row 19
    present = np.ones(20, dtype=bool)
    idx, val, n, total, nxt = pkg.page_after(y, present, 5)
    assert (n, total, nxt) == (5, 20, (15, bits_of(16.0), AFTER)) and idx.tolist() == [19, 18, 17, 16, 15]
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (5, bits_of(6.0), AFTER))
    assert (n, total) == (5, 5) and idx.tolist() == [4, 3, 2, 1, 0] and nxt == (0, 0, END)  # total == k exactly: no page follows
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (6, bits_of(7.0), AFTER))
    assert (n, total, nxt) == (5, 6, (1, bits_of(2.0), AFTER))  # one more row than a page: AFTER(the last real entry)
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, nxt)
    assert (n, total, nxt) == (1, 1, (0, 0, END)) and idx.tolist() == [0, 0, 0, 0, 0] and val[0] == 1.0 and np.all(val[1:] == 0)
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (0, bits_of(1.0), AFTER))
    assert (n, total, nxt) == (0, 0, (0, 0, END))  # nothing behind the last row
    idx, val, n, total, nxt = pkg.page_after(y, np.zeros(20, dtype=bool), 5)
    assert (n, total, nxt) == (0, 0, (0, 0, END)) and np.all(idx == 0)  # START over nothing
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (111, bits_of(11.0), AFTER), first_row=100)
    assert (n, total) == (5, 11) and idx.tolist() == [110, 109, 108, 107, 106]  # global ids: row 110 scores 11.0 and 110 < 111
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (10, bits_of(11.0), AFTER), first_row=100)
    assert (n, total) == (5, 10) and idx.tolist() == [109, 108, 107, 106, 105]  # ... and 110 is not below 10


def test_signed_zeros_and_minus_infinity_like_the_device(pkg):
    y = np.array([-0.0, 0.0, -np.inf, 1.0, -np.inf], dtype=np.float32)
    present = np.ones(5, dtype=bool)
    idx, val, n, total, nxt = pkg.page_after(y, present, 5)
    assert n == total == 2 and idx[:2].tolist() == [3, 1]  # -0.0 sorts below +0.0 = min_score by the order key
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, None, -np.inf)
    assert n == total == 3 and idx[:3].tolist() == [3, 1, 0] and val[2].view(np.uint32) == 0x80000000  # -inf is never eligible
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (1, 0x00000000, AFTER), -np.inf)
    assert n == total == 1 and idx[0] == 0 and val[0].view(np.uint32) == 0x80000000  # behind (row 1, +0.0): -0.0 alone
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (7, 0x80000000, AFTER), -np.inf)
    assert n == total == 1 and idx[0] == 0  # a cursor at -0.0 with a larger row id: row 0 is behind it ...
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (0, 0x80000000, AFTER), -np.inf)
    assert n == total == 0 and nxt == (0, 0, END)  # ... and not behind itself
    idx, val, n, total, nxt = pkg.page_after(y, present, 5, (9, 0xFF800000, AFTER), -np.inf)
    assert n == total == 0  # a cursor at -inf: nothing is eligible behind it
