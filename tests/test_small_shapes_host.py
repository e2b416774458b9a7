"""The fixtures of test_gpu_small_shapes.py (tests/small_shapes.py), checked without a device.

A. The short-run labelings reach every situation of a lane of group_best_kernel: the three coverage conditions of small_shapes'
   docstring are asserted here from labels and scores alone, and so is what the GPU test takes for granted about the scores (exact,
   distinct integers: the oracle over the packed stream gives exactly the matrix' values) and about the mask (groups end empty).
B. On all 18 tiny shapes, at 4 and 8 entries per lane, the references the GPU test compares with agree among themselves: the packer
   and the order-matched oracle with fp64 sums; page_after walked to END with oracle.select_topk; collapse_topk, facet_counts and
   boosted_matches with the same ranking; the Packed twins with the contract's restatements over the oracle's scores and the COO."""
import itertools

import numpy as np
import pytest

import small_shapes as S
from support import bits, present

KINDS = (0, 1, 2)
NINF = float("-inf")
END = 2


# ---- A ----------------------------------------------------------------------------------------------------------------------------
def test_short_runs_reach_every_lane_situation(pkg):
    seen, pairs, spans = S.coverage(pkg)
    every = list(itertools.product((False, True), repeat=5))
    counts = {t: seen.get(t, 0) for t in every}
    print("occurrences per (b01, b12, b23, joins, continues):", counts)
    assert min(counts.values()) >= 4, ("condition 1", {t: n for t, n in counts.items() if n < 4})
    missing = [(t, p) for t in every for p in range(S.LANE_ROWS) if (t, p) not in pairs]
    print("pairs reached:", len(every) * S.LANE_ROWS - len(missing), "spans per matrix:", [len(s) for s in spans])
    assert not missing, ("condition 2", missing)
    flat = [s for per in spans for s in per]
    assert len(flat) >= 4 and any(r < b for b, r in flat) and any(r >= b for b, r in flat), ("condition 3", spans)
    assert {rows % 4 for rows in S.RUN_ROWS} == {0, 1, 2, 3} and S.RUN_C8 in S.RUN_ROWS


@pytest.mark.parametrize("rows", S.RUN_ROWS)
def test_short_run_fixture(pkg, oracle, rows):
    m = S.run_matrix(pkg, rows)
    labels, run = S.run_labels(rows)
    assert np.array_equal(np.bincount(m.row, minlength=rows), np.ones(rows)) and m.cols == S.RUN_COLS
    assert np.array_equal(np.sort(m.val), np.arange(1, rows + 1, dtype=np.float32))
    ln = np.bincount(run)
    assert set(ln[:-1].tolist()) == set(S.RUN_LENGTHS) and np.all(labels == run % S.N_GROUPS) and S.N_GROUPS <= S.RUN_K
    n_runs = np.bincount(labels[np.concatenate([[True], run[1:] != run[:-1]])], minlength=S.N_GROUPS)
    assert np.all(n_runs >= 1) and (n_runs >= 2).mean() > 0.9, "most groups own two or more separate runs"
    # every score is the row's value times the scale, whatever the layout sums: the order-matched oracle says the same
    for c_lane in (4, 8):
        packed = pkg.Packed(m, k=S.RUN_K, nnz_per_lane=c_lane)
        for scale in (1.0, 2.0, 0.5):
            y, pres = oracle.packed_scores(packed.raw(), np.full(S.RUN_COLS, scale, dtype=np.float32), rows, c_lane)
            assert np.all(pres) and np.array_equal(bits(y), bits(S.run_scores(m, scale)))
    y = S.run_scores(m)
    allow = S.run_mask(rows, labels, run)
    assert 0.25 < 1 - allow.mean() < 0.35
    gone = np.setdiff1d(np.arange(run.max() + 1), run[allow])
    assert gone.size > 50, "whole runs are removed"
    full, part = pkg.collapse_topk(y, np.ones(rows, dtype=bool), labels, S.RUN_K, NINF), pkg.collapse_topk(y, allow, labels, S.RUN_K, NINF)
    assert full[3] == S.N_GROUPS and 700 < part[3] < S.N_GROUPS, "groups end empty under the mask"
    lost = np.setdiff1d(full[0][:full[3]], part[0][:part[3]])
    assert lost.size > 100, "groups lose their best row under the mask"
    b = S.tile_bias(rows)
    assert np.count_nonzero(b) == (rows + S.TILE - 1) // S.TILE and np.all(np.add.reduceat(b != 0, np.arange(0, rows, S.TILE)) == 1)
    assert np.array_equal((y + b).astype(np.float64), y.astype(np.float64) + b.astype(np.float64)) and y.max() < S.LIFT


# ---- B ----------------------------------------------------------------------------------------------------------------------------
def test_tiny_shapes_are_the_listed_ones(pkg):
    assert len(S.TINY) == 18
    for name, (ln, cols) in S.TINY.items():
        m = S.tiny(pkg, name)
        assert m.rows == len(ln) and m.cols == cols and np.array_equal(np.bincount(m.row, minlength=m.rows), ln)
        assert not np.any(m.val == 0) and (m.row.size < 4 or (np.any(m.val < 0) and np.any(m.val > 0)))
        for r in range(m.rows):
            c = m.col[m.row == r]
            assert np.all(c[1:] > c[:-1]), "columns sorted and distinct per row"
        ks = S.tiny_ks(m)
        assert ks[0] == 1 and max(ks) <= S.MAX_K and ks[-1] == min(S.MAX_K, m.rows + 47)
    assert {len(S.TINY[f"rows{r}"][0]) for r in S.CYCLE_ROWS} == set(S.CYCLE_ROWS)


def _walk(pkg, y, pres, k, first_row):
    """page_after from START to END: (rows of all pages in order, pages)."""
    cursor, out, pages = None, [], 0
    while True:
        idx, val, n, total, nxt = pkg.page_after(y, pres, k, cursor, NINF, first_row)
        if pages == 0:
            first_total = total
        assert total == first_total - len(out) and n == min(k, total)
        assert np.all(idx[n:] == 0) and np.all(bits(val[n:]) == 0)
        out += idx[:n].tolist()
        pages += 1
        cursor = nxt
        if nxt[2] == END:
            return np.array(out, dtype=np.int64), pages
        assert pages <= first_total, "the walk does not end"


@pytest.mark.parametrize("c_lane", [4, 8])
@pytest.mark.parametrize("name", list(S.TINY))
def test_references_agree_on_the_tiny_shapes(pkg, oracle, name, c_lane):
    L = pkg._lib
    m = S.tiny(pkg, name)
    rows, cols = m.rows, m.cols
    pres = present(m)
    n_pres = int(pres.sum())
    packed = pkg.Packed(m, k=16, nnz_per_lane=c_lane)
    assert packed.info()["packet_entries"] == 64 * c_lane and packed.info()["rows"] == rows
    dr, dc, dv = packed.decode()
    assert np.array_equal(dr, m.row) and np.array_equal(dc, m.col) and np.array_equal(bits(dv), bits(m.val))
    xs = S.tiny_vectors(cols)
    ys = []
    for x in xs:
        y, p = oracle.packed_scores(packed.raw(), x, rows, c_lane)
        assert np.array_equal(p.astype(bool), pres) and np.all(bits(y[~pres]) == 0)
        y64 = np.zeros(rows)
        np.add.at(y64, m.row, m.val.astype(np.float64) * x[m.col].astype(np.float64))
        assert np.all(np.abs(y - y64) <= 1e-4 * np.maximum(1.0, np.abs(y64))), "the oracle's scores against fp64 sums"
        ys.append(y)
    y = ys[0]
    # rankings: oracle.select_topk of all rows is the order; the walks, the collapse, the range and the facets restate it
    for first_row in (0, S.FIRST_ROW):
        ei, ev = oracle.select_topk(y, pres.astype(np.uint8), max(rows, 1), NINF, first_row)
        order = ei[:n_pres].astype(np.int64)
        assert np.all(ei[n_pres:] == 0) and np.all(bits(ev[n_pres:]) == 0)
        assert np.array_equal(np.sort(order - first_row), np.flatnonzero(pres))
        for k in S.tiny_ks(m):
            got, pages = _walk(pkg, y, pres, k, first_row)
            assert np.array_equal(got, order), (k, "the pages of a walk add up to the rows with entries, in select_topk's order")
            assert pages == max(1, -(-n_pres // k))
            ti, tv = oracle.select_topk(y, pres.astype(np.uint8), k, NINF, first_row)
            assert np.array_equal(ti[:min(k, n_pres)], ei[:min(k, n_pres)]) and np.array_equal(bits(tv[:min(k, n_pres)]), bits(ev[:min(k, n_pres)]))
        ci, cv, cg, cn = pkg.collapse_topk(y, pres, np.arange(rows), max(rows, 1), NINF, first_row)
        assert cn == n_pres and np.array_equal(ci, ei) and np.array_equal(bits(cv), bits(ev)) and np.array_equal(cg[:cn], order - first_row)
        wi, wv, wn = pkg.boosted_matches(y, pres, NINF, None, None, None, first_row)
        assert wn == n_pres and np.array_equal(wi, ei[:n_pres]) and np.array_equal(bits(wv), bits(ev[:n_pres]))
        for name_l, (labels, n_groups) in S.tiny_labelings(rows).items():
            gi, gv, gg, gn = pkg.collapse_topk(y, pres, labels, max(rows, 1), NINF, first_row)
            assert gn == np.unique(labels[pres]).size
            fc, fi, fv, ft = pkg.facet_counts(y, pres, labels, n_groups, NINF, first_row)
            assert ft == n_pres and np.array_equal(fc, np.bincount(labels[pres], minlength=n_groups))
            # a group's representative is its facet bin's best match
            assert np.array_equal(fi[gg[:gn]], gi[:gn]) and np.array_equal(bits(fv[gg[:gn]]), bits(gv[:gn])), name_l
    if n_pres:
        best = float(y[pres].max())
        assert pkg.boosted_matches(y, pres, best)[2] == int((y[pres] == np.float32(best)).sum()) >= 1
        assert pkg.boosted_matches(y, pres, float(np.nextafter(np.float32(best), np.float32(np.inf))))[2] == 0
    # the Packed twins
    near_xs = np.random.default_rng(rows).standard_normal((17, cols)).astype(np.float32)
    near_y = np.stack([oracle.packed_scores(packed.raw(), x, rows, c_lane)[0] for x in near_xs])
    for count in (1, 5, 17):
        al, ab = packed.assign(near_xs[:count])
        wl, wb = pkg.nearest(near_y[:count])
        assert np.array_equal(al, wl) and np.array_equal(bits(ab), bits(wb)), (count, "Packed.assign")
        for n in (1, 2, 3, 4):
            gl, gs = packed.nearest(near_xs[:count], n)
            wl, ws = pkg.nearest_n(near_y[:count], n)
            assert np.array_equal(gl, wl) and np.array_equal(bits(gs), bits(ws)), (count, n, "Packed.nearest")
    st = [packed.row_stats(kind) for kind in (0, 1, 2, 3)]
    assert np.array_equal(st[0], np.bincount(m.row, minlength=rows).astype(np.float32))
    l1 = np.zeros(rows)
    np.add.at(l1, m.row, np.abs(m.val.astype(np.float64)))
    l2 = np.zeros(rows)
    np.add.at(l2, m.row, m.val.astype(np.float64) ** 2)
    assert np.allclose(st[1], l1, rtol=1e-4, atol=0) and np.allclose(st[2], l2, rtol=1e-4, atol=0)
    assert np.array_equal(bits(st[3]), bits(pkg.inv_l2(st[2])))
    for x, yq in zip(xs, ys):
        assert np.array_equal(bits(packed.score_rows(x, np.arange(rows))), bits(yq)), "Packed.score_rows"
    starts = np.searchsorted(m.row, np.arange(rows + 1))
    for r in np.flatnonzero(pres):
        c, v = packed.get_row(int(r))
        assert np.array_equal(c, m.col[starts[r]:starts[r + 1]]) and np.array_equal(bits(v), bits(m.val[starts[r]:starts[r + 1]])), "Packed.get_row"
    for kind in KINDS:
        assert np.array_equal(packed.col_stats(kind).view(np.uint32), pkg.col_stats(m, kind).view(np.uint32)), "Packed.col_stats"
    e = packed.sums_exponent()
    assert e == pkg.sums_exponent(m)
    for n_bins in (1, 3, rows + 5):
        labels = (np.arange(rows) % 3).astype(np.uint32)
        want = pkg.label_sums(m, labels, n_bins, e)
        sums, f = packed.label_sums(labels, n_bins, e, L.SUMS_FLOAT)
        assert np.array_equal(sums, want), "Packed.label_sums"
        assert np.array_equal(bits(f), bits(pkg.close_sums(want, e, L.SUMS_FLOAT))), "the closing rule"
    packed.close()
