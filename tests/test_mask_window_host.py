"""The fixtures of the allow-mask tests (tests/dense_ends.py), checked without a device.

1. What the packets of dense_ends.matrix() look like, from Packed(...).raw(): the properties test_gpu_mask_window.py relies on to reach
   the further-words loop of mask_rows / mask_entries, the packets without a row end and the clamped last word.
2. An expectation for the scores that shares nothing with the project's summation code: a row of at most two entries scores
   fl(v0 x0) or fl(fl(v0 x0) + fl(v1 x1)) in plain numpy float32, and the order-matched oracle agrees with that bit for bit. That is
   most of the fixture (every one-entry row, the short rows).
3. The host twins under the fixture's masks: Packed.nearest and Packed.col_stats against host.nearest_n and host.col_stats on the COO,
   with clean mask words and with every bit at and beyond `rows` set: identical."""
import numpy as np
import pytest

import dense_ends
from support import bits

CASES = [(rows, variant) for rows in dense_ends.ROWS for variant in dense_ends.VARIANTS]
KINDS = (0, 1, 2)


def _xs(count, seed):
    return np.random.default_rng(seed).standard_normal((count, dense_ends.COLS)).astype(np.float32)


@pytest.mark.parametrize("c_lane", [4, 8])
@pytest.mark.parametrize("rows,variant", CASES)
def test_fixture_properties(pkg, rows, variant, c_lane):
    m = dense_ends.matrix(pkg, rows, variant)
    ln = np.bincount(m.row, minlength=rows)
    assert m.rows == rows and m.cols == dense_ends.COLS and np.array_equal(ln, dense_ends.lengths(rows, variant))
    assert np.all(ln[:dense_ends.ONES] == 1) and dense_ends.ONES >= 600
    assert np.all(ln[dense_ends.ONES:dense_ends.ONES + dense_ends.EMPTY] == 0) and dense_ends.EMPTY >= 300
    assert ln[dense_ends.LONG_ROW] == dense_ends.LONG == 700 and np.all(ln[dense_ends.LONG_ROW + 1:dense_ends.ORDINARY] == 1)
    assert ln[-1] == (0 if variant == "last_empty" else dense_ends.FULL)
    assert np.any(m.val < 0) and np.any(m.val > 0)
    # the layout an engine created from the COO streams (a stream this short is cut the same for every partition hint above its packets)
    t = dense_ends.packet_table(pkg.Packed(m, k=16, nnz_per_lane=c_lane), m)
    assert any(n >= 200 for _, n, _, _ in t), "no packet ends at least 200 rows"
    assert any(n and ((rb + n - 1) >> 5) - (rb >> 5) + 1 >= 5 for rb, n, _, _ in t), "no packet's rows span at least 5 mask words"
    assert any(n == 0 for _, n, _, _ in t), "no packet without a row end"
    assert any(rb % 32 == 31 for rb, _, _, _ in t), "no packet starts at a row with rb % 32 == 31"
    assert any(rb % 32 == 0 for rb, _, _, _ in t), "no packet starts at a row with rb % 32 == 0"
    assert t[-1][3] > 0, "the last partition has no trailing padding"
    i = dense_ends.DENSE_LAST[c_lane // 8]
    assert any(rb + n - 1 == i and n >= 200 for rb, n, _, _ in t), f"row {i} is not the last row a dense packet ends"
    # the layout of the prepacked engines: partitions of many packets, so a packet that ends more than two mask words of rows also holds
    # entries of a row that goes on in the next packet, and that row opens a mask word: the one word mask_entries reads beyond mask_rows
    packed = pkg.Packed(m, k=16, nnz_per_lane=c_lane, n_wave_partitions=dense_ends.PREPACKED_PARTITIONS)
    assert packed.info()["n_wave_partitions"] == dense_ends.PREPACKED_PARTITIONS
    t = dense_ends.packet_table(packed, m)
    hit = [(rb, n) for rb, n, cont, _ in t if cont and (rb + n) % 32 == 0 and ((rb + n) >> 5) >= (rb >> 5) + 2]
    assert hit, "no packet whose continuing row opens a mask word behind the two prefetched ones"
    assert any(rb + n == dense_ends.ORDINARY for rb, n in hit), "the first ordinary row was laid out to be that row"


@pytest.mark.parametrize("c_lane", [4, 8])
@pytest.mark.parametrize("rows,variant", CASES[:2])
def test_short_rows_score_what_plain_float32_arithmetic_gives(pkg, oracle, rows, variant, c_lane):
    m = dense_ends.matrix(pkg, rows, variant)
    x = dense_ends.vector()
    for parts in (4096, dense_ends.PREPACKED_PARTITIONS):
        packed = pkg.Packed(m, k=16, nnz_per_lane=c_lane, n_wave_partitions=parts)
        y, present = oracle.packed_scores(packed.raw(), x, rows, c_lane)
        ln = np.bincount(m.row, minlength=rows)
        assert np.array_equal(present.astype(bool), ln > 0)
        first = np.concatenate([[0], np.cumsum(ln)])[:-1]
        p = (m.val * x[m.col]).astype(np.float32)  # one rounding per product
        one, two = np.flatnonzero(ln == 1), np.flatnonzero(ln == 2)
        assert one.size >= dense_ends.ONES + dense_ends.AFTER_LONG and two.size >= 40
        assert np.array_equal(bits(y[one]), bits(p[first[one]])), "a one-entry row does not score fl(v0 x0)"
        assert np.array_equal(bits(y[two]), bits(p[first[two]] + p[first[two] + 1])), "a two-entry row does not score fl(fl(v0 x0) + fl(v1 x1))"
        assert np.all(bits(y[ln == 0]) == 0), "a row without entries does not score +0.0"


def _twins(pkg, oracle, m, c_lane, parts, masks, label):
    rows = m.rows
    packed = pkg.Packed(m, k=16, nnz_per_lane=c_lane, n_wave_partitions=parts)
    xs = _xs(5, rows)
    y = np.stack([oracle.packed_scores(packed.raw(), x, rows, c_lane)[0] for x in xs])
    total = np.bincount(m.row, minlength=rows)
    for name, allow in masks.items():
        for dirty in (False, True):
            w = dense_ends.words(pkg, rows, allow, dirty)
            assert (dirty and rows % 32 != 0) == (not np.array_equal(w, pkg.row_mask(rows, allow)))  # (rows % 32 == 0: no such bits)
            for n in (1, 4):
                gl, gs = packed.nearest(xs, n, w)
                wl, ws = pkg.nearest_n(y, n, allow)
                assert np.array_equal(gl, wl) and np.array_equal(bits(gs), bits(ws)), f"{label}/{name}/dirty={dirty}: Packed.nearest n={n}"
            for kind in KINDS:
                got, want = packed.col_stats(kind, w), pkg.col_stats(m, kind, allow)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{label}/{name}/dirty={dirty}: Packed.col_stats kind {kind}"
            assert int(packed.col_stats(0, w).sum()) == int(total[allow].sum()), f"{label}/{name}: a placeholder or padding was counted"


@pytest.mark.parametrize("c_lane", [4, 8])
@pytest.mark.parametrize("rows,variant", CASES)
def test_host_twins_under_the_masks(pkg, oracle, rows, variant, c_lane):
    m = dense_ends.matrix(pkg, rows, variant)
    for parts in (4096, dense_ends.PREPACKED_PARTITIONS):
        _twins(pkg, oracle, m, c_lane, parts, dense_ends.masks(rows), f"{rows}/{variant}/C={c_lane}/P={parts}")


@pytest.mark.parametrize("rows", dense_ends.TINY_ROWS)
def test_host_twins_on_the_tiny_matrices(pkg, oracle, rows):
    m = dense_ends.tiny(pkg, rows)
    assert m.rows == rows and m.row.size >= 1 and (rows == 1 or np.any(np.bincount(m.row, minlength=rows) == 0))
    assert pkg.row_mask(rows, None).size == (1 if rows <= 32 else 2 if rows <= 64 else 3)
    for c_lane in (4, 8):
        _twins(pkg, oracle, m, c_lane, 4096, dense_ends.tiny_masks(rows), f"tiny {rows}/C={c_lane}")
