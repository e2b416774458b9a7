"""Short label runs through the group fold, and every call on tiny matrices (tests/small_shapes.py), on the MI355X.

A. group_best_kernel (kernels/group_select.hpp) on labelings of short runs, which reach each of a lane's 32 situations -- three
   in-lane boundaries, joins, continues -- with the run's best row at each of the four in-lane positions, and runs that span the
   256-row tile (test_small_shapes_host.py asserts that from labels and scores). One entry per row, the values a permutation of
   1 .. rows and queries of ones: the scores are exact integers, the expectation host.collapse_topk over them. 900 groups <= k = 1024:
   every group's representative is compared. enqueue_grouped without and with a mask that empties groups, run_grouped,
   enqueue_boosted_grouped with w = -1 (each group's lowest row) and with a bias that lifts one row per tile, three queries in one call.

B. 18 shapes of 1 .. 1025 rows (one packet and one partition; rows < 4; rows around 64, 256 and 1024; empty rows in front, at the
   end; one row that spans packets) through every call, on engines of k = 1, k = the rows with entries and k = rows + 47 (at most
   1024), 4 and 8 entries per lane, first_row = 5000, and one engine created with multi_q = 2. Everything is compared bit for bit:
   scores with the order-matched oracle's over the engine's own layout (support.Layout), the contract with the restatement each
   call's own test file uses. Outputs sit between guard zones; checks_failed, late_repairs and single_repairs do not move.

One module-scoped fixture per part holds the engines of one shape: pytest groups the tests by it. The conftest syncs torch only for
the older enqueue names: the other calls go through helpers that call torch.cuda.synchronize() themselves.

Evidence that the tests bite. Each mutation below was applied to a copy of the tree, the library built from it and this file run once
against it (TKSPMV_LIB); with the unchanged library all 136 tests pass. The mutations change values only.
  1. group_best_kernel without the "rows 1 and 2" offer. Failed: test_short_runs_grouped and test_short_runs_boosted_grouped on all
     five cases (n = 894 .. 898 instead of 900: groups whose runs are all of that kind vanish). No tiny test: the labelings r // 3,
     r % 2 and identity have no two-row run at lane offset 1.
  2. joins = (below == lab[0]) without the lane != 0 test. NOT caught, all 136 pass -- and no test can catch it: the mutant computes
     the same maxima. In lane 0 __shfl_up(.., 1) returns the lane's own lab[3], so the mutant's lane 0 "joins" exactly when its first
     and last label agree. Without a boundary in the lane that only clears its head flag, which no lane reads (the scan takes
     from lane - d only for lane >= d); with one, it offers max(H, carried) where carried is lane 0's own T, the maximum of a run
     of the very label the offer goes to. A lane-level model of the kernel on 3000 random tiles (labels that repeat within and
     across lanes, ineligible rows) gave the same group maxima with and without the test, and the true ones. The test in the
     kernel is redundant, not wrong; it stays.
  3. The split offers H instead of group_max(H, carried). Failed: both short-run tests on all five cases (row ids), and
     test_tiny_grouped (labels r // 3, plain and boosted) on empty_front and every shape of 31 rows and more.
  4. after_finish_kernel: AFTER for total >= k. Failed: test_tiny_walks on all 18 shapes (the k = 1 walk's last page, and
     k = the eligible rows, answer AFTER(last entry) where page_after says END).
  5. boosted_hits_kernel counts a tile's matches from three of a lane's four rows. Failed: test_tiny_range_and_facets
     (boosted_range; counts of 19 for 25, 614 for 819, ...) on empty_front and every shape of 31 rows and more; the shapes below
     have no row at an in-lane offset 3 with entries. enqueue_range has a kernel of its own and passes.

Wall time on the MI355X, both files in one run on the unchanged library: this file 8.1 s (136 tests), test_gpu_mask_window.py
3.9 s (72 tests).
"""
import numpy as np
import pytest

import small_shapes as S
import support
from support import GUARD, GuardedOut, Layout, PageOut, bits
from test_gpu_boost import _same as _same_page
from test_gpu_boost_forms import _facets, _grouped, _range, _same_facets, _same_grouped
from test_gpu_label_sums import _enqueue as _sums_enqueue, _sinks
from test_gpu_match import _expect as _match_expect, _match, _same as _same_match
from test_gpu_score_rows import _run as _score_rows
from test_gpu_similar import _run_row_vectors

pytestmark = pytest.mark.gpu

END = 2
NINF = float("-inf")
NINF_BITS = 0xFF800000
NONE = 0xFFFFFFFF
OUTSIDE = 0xFFFFFFFF
COUNTERS = ("checks_failed", "late_repairs", "single_repairs")


class TopkOut(GuardedOut):
    COLUMNS = (("dev_idx", "k", "int32"), ("dev_val", "k", "float32"))


def _guarded(torch, **columns):
    """One call's outputs between guard zones: keyword -> (words, dtype name)."""
    return type("Out", (GuardedOut,), {"COLUMNS": tuple((name, n, dt) for name, (n, dt) in columns.items())})(torch, 1, 0)


def _dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def _dev_f32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).copy()).cuda()


class _Counters:
    """with _Counters(eng): the three repair counters are what they were."""
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.c0 = self.eng.debug_counters()

    def __exit__(self, et, ev, tb):
        if et is None:
            c1 = self.eng.debug_counters()
            assert all(self.c0[c] == c1[c] for c in COUNTERS), ("a repair counter moved", {c: (self.c0[c], c1[c]) for c in COUNTERS})


def _same_topk(got_idx, got_val, want, what):
    assert np.array_equal(np.asarray(got_idx).view(np.uint32), want[0]), (what, "row ids")
    assert np.array_equal(bits(got_val), bits(want[1])), (what, "score bits")


# ==== A: short label runs ==============================================================================================================
RUN_CASES = [(rows, 4) for rows in S.RUN_ROWS] + [(S.RUN_C8, 8)]


class _Runs:
    def __init__(self, pkg, torch, rows, c_lane):
        self.pkg, self.torch, self.rows = pkg, torch, rows
        self.m = S.run_matrix(pkg, rows)
        self.labels, self.run = S.run_labels(rows)
        self.eng = pkg.SpMV(self.m.row, self.m.col, self.m.val, rows, S.RUN_COLS, k=S.RUN_K, device=0, nnz_per_lane=c_lane, min_score=NINF)
        assert self.eng.info()["packet_entries"] == 64 * c_lane
        self.eng.set_groups(self.labels, S.N_GROUPS)
        self.scales = (1.0, 2.0, 0.5)
        self.xs = np.stack([np.full(S.RUN_COLS, s, dtype=np.float32) for s in self.scales])
        self.ys = [S.run_scores(self.m, s) for s in self.scales]
        self.dxs = _dev_f32(torch, self.xs)
        self.allow = S.run_mask(rows, self.labels, self.run)
        self.dmask = _dev_u32(torch, pkg.row_mask(rows, self.allow))
        self.every = np.ones(rows, dtype=bool)

    def want(self, scores, ok):
        return self.pkg.collapse_topk(scores, ok, self.labels, S.RUN_K, NINF, 0)


@pytest.fixture(scope="module", params=RUN_CASES, ids=[f"{r}-C{c}" for r, c in RUN_CASES])
def runs(request, pkg):
    import torch
    r = _Runs(pkg, torch, *request.param)
    yield r
    r.eng.close()


def test_short_runs_grouped(runs):
    R, torch, eng = runs, runs.torch, runs.eng
    with _Counters(eng):
        got, = _grouped(eng, torch, R.dxs, 1, plain=True)
        want = R.want(R.ys[0], R.every)
        assert want[3] == S.N_GROUPS
        _same_grouped(got, want, "enqueue_grouped")
        got, = _grouped(eng, torch, R.dxs, 1, mask=R.dmask, plain=True)
        want_m = R.want(R.ys[0], R.allow)
        assert 0 < want_m[3] < S.N_GROUPS and np.all(want_m[2][want_m[3]:] == NONE)
        _same_grouped(got, want_m, "enqueue_grouped under the mask")
        for q, g in enumerate(_grouped(eng, torch, R.dxs, 3, plain=True)):
            _same_grouped(g, R.want(R.ys[q], R.every), ("three queries", q))
        for q, g in enumerate(_grouped(eng, torch, R.dxs, 3, mask=R.dmask, plain=True)):
            _same_grouped(g, R.want(R.ys[q], R.allow), ("three queries under the mask", q))
        eng.reset(R.xs[0])
        for allow, w in ((None, want), (R.allow, want_m)):
            val, idx, grp = eng.run_grouped(allow=allow)
            n = w[3]
            assert idx.size == n and np.array_equal(idx, w[0][:n]) and np.array_equal(bits(val), bits(w[1][:n])) and np.array_equal(grp, w[2][:n]), "run_grouped"
        eng.set_filter(None)


def test_short_runs_boosted_grouped(runs):
    R, torch, eng, pkg = runs, runs.torch, runs.eng, runs.pkg
    minus, lift = np.full(R.rows, -1.0, dtype=np.float32), S.tile_bias(R.rows)
    dminus, dlift = _dev_f32(torch, minus), _dev_f32(torch, lift)
    with _Counters(eng):
        sb = pkg.boost_scores(R.ys[0], minus, None)
        assert np.array_equal(sb, -R.ys[0])
        got, = _grouped(eng, torch, R.dxs, 1, w=dminus)
        want = R.want(sb, R.every)
        lowest = np.full(S.N_GROUPS, np.inf)
        np.minimum.at(lowest, R.labels, R.ys[0])
        assert want[3] == S.N_GROUPS and np.array_equal(-want[1][:S.N_GROUPS], lowest[want[2][:S.N_GROUPS]]), "each group's lowest-scoring row"
        _same_grouped(got, want, "w = -1")
        got, = _grouped(eng, torch, R.dxs, 1, w=dminus, mask=R.dmask)
        _same_grouped(got, R.want(sb, R.allow), "w = -1 under the mask")
        sb = pkg.boost_scores(R.ys[0], None, lift)
        got, = _grouped(eng, torch, R.dxs, 1, b=dlift)
        want = R.want(sb, R.every)
        n_lifted = np.unique(R.labels[lift != 0]).size  # (two lifted rows of one group: one representative)
        assert n_lifted > 10 and np.all(lift[want[0][:n_lifted]] == S.LIFT) and not np.any(lift[want[0][n_lifted:]])
        _same_grouped(got, want, "one lifted row per tile")
        for q, g in enumerate(_grouped(eng, torch, R.dxs, 3, w=dminus, b=dlift)):
            _same_grouped(g, R.want(pkg.boost_scores(R.ys[q], minus, lift), R.every), ("three boosted queries", q))


# ==== B: tiny matrices =================================================================================================================
class _Engine:
    """One engine of a tiny shape, with the order-matched oracle's scores of its own layout for the shape's vectors."""
    def __init__(self, pkg, oracle, T, spec):
        c_lane, k, first_row, multi_q = spec
        m = T.m
        self.tag = f"{T.name}/C={c_lane}/k={k}/first_row={first_row}/multi_q={multi_q}"
        self.k, self.first_row = k, first_row
        # (a status other than OK raises here: every tiny engine must be created)
        self.eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, nnz_per_lane=c_lane, min_score=NINF, first_row=first_row, multi_q=multi_q)
        self.info = self.eng.info()
        assert self.info["packet_entries"] == 64 * c_lane, self.tag
        self.layout = Layout(pkg, self.eng, m)
        self.twin = self.layout._keep
        scored = [self.layout.scores(oracle, x) for x in T.xs]
        assert all(np.array_equal(p, T.present) for _, p in scored), self.tag
        self.ys = [y for y, _ in scored]
        self.sb = [pkg.boost_scores(y, T.w, T.b) for y in self.ys]
        self.sb_ok = [T.present & (s > -np.inf) for s in self.sb]
        self.near_y = np.stack([self.layout.scores(oracle, x)[0] for x in T.near_xs])


class _Tiny:
    def __init__(self, pkg, oracle, torch, name):
        self.pkg, self.oracle, self.torch, self.name = pkg, oracle, torch, name
        self.m = m = S.tiny(pkg, name)
        self.rows, self.cols = m.rows, m.cols
        self.present = support.present(m)
        self.n_present = int(self.present.sum())
        self.xs = S.tiny_vectors(m.cols)
        self.dxs = _dev_f32(torch, self.xs)
        self.dx4 = _dev_f32(torch, np.tile(self.xs[0], (4, 1)))
        rng = np.random.default_rng(m.rows + 1)
        self.w, self.b = rng.uniform(0.5, 2.0, m.rows).astype(np.float32), rng.uniform(-1.0, 1.0, m.rows).astype(np.float32)
        self.dw, self.db = _dev_f32(torch, self.w), _dev_f32(torch, self.b)
        self.minus = np.full(m.rows, -1.0, dtype=np.float32)
        self.dminus = _dev_f32(torch, self.minus)
        self.near_xs = np.random.default_rng(m.rows).standard_normal((17, m.cols)).astype(np.float32)
        self.dnear = _dev_f32(torch, self.near_xs)
        self.labels3 = (np.arange(m.rows) % 3).astype(np.uint32)
        self.dlabels3 = _dev_u32(torch, self.labels3)
        self.engines = []
        for spec in S.tiny_engines(m):
            self.engines.append(_Engine(pkg, oracle, self, spec))

    def close(self):
        for E in self.engines:
            E.eng.close()


@pytest.fixture(scope="module", params=list(S.TINY))
def tiny(request, pkg, oracle):
    import torch
    T = _Tiny(pkg, oracle, torch, request.param)
    yield T
    T.close()


def _thresholds(scores, ok):
    """-inf, 0, the best score, just above the best score."""
    best = np.float32(scores[ok].max())
    return [NINF, 0.0, float(best), float(np.nextafter(best, np.float32(np.inf)))]


def test_tiny_engines(tiny):
    """The engines of a shape: the three k, 8 entries per lane and first_row where the shape has them, one with multi_q."""
    T = tiny
    ks = S.tiny_ks(T.m)
    assert {E.k for E in T.engines} == set(ks) and ks[0] == 1 and T.n_present >= 1
    assert (T.rows in S.C8_ROWS) == any(E.info["packet_entries"] == 512 for E in T.engines)
    assert (T.rows in S.FIRST_ROW_ROWS) == any(E.first_row == S.FIRST_ROW for E in T.engines)
    assert len(T.engines) == len(S.tiny_engines(T.m))
    for E in T.engines:
        assert E.info["rows"] == T.rows and E.info["cols"] == T.cols, E.tag


def test_tiny_topk(tiny):
    """tkspmv_run, enqueue_batch, enqueue_multi, enqueue_filtered under four masks, similar."""
    T, torch, oracle = tiny, tiny.torch, tiny.oracle
    pres8 = T.present.astype(np.uint8)
    for E in T.engines:
        eng, k = E.eng, E.k
        wants = [oracle.select_topk(y, pres8, k, NINF, E.first_row) for y in E.ys]
        n_real = min(k, T.n_present)
        assert all(np.all(w[0][n_real:] == 0) and np.all(bits(w[1][n_real:]) == 0) for w in wants)
        with _Counters(eng):
            for q in range(3):
                eng.reset(T.xs[q])
                eng()
                val, idx = eng.read_result()
                assert idx.size == k
                _same_topk(idx, val, wants[q], (E.tag, "tkspmv_run", q))
            out = TopkOut(torch, 3, k)
            eng.enqueue_batch(T.dxs.data_ptr(), 3, **out.ptrs())
            eng.synchronize()
            res = out.read()
            for q in range(3):
                _same_topk(res["dev_idx"][q], res["dev_val"][q], wants[q], (E.tag, "enqueue_batch", q))
            if E.info["multi_q"] != 0:
                # the multi-query kernel sums a row in its own entry order, in segments of 64 entries, not in packet order: its lists
                # are the exact selection over oracle.scores_f32_segmented (test_gpu_engine.py), last-bit differences to the others'
                out = TopkOut(torch, 3, k)
                eng.enqueue_multi(T.dxs.data_ptr(), 3, **out.ptrs())
                eng.synchronize()
                res = out.read()
                for q in range(3):
                    y, p = oracle.scores_f32_segmented(T.m.row, T.m.col, T.m.val, T.xs[q], T.rows)
                    assert np.array_equal(p.astype(bool), T.present)
                    _same_topk(res["dev_idx"][q], res["dev_val"][q], oracle.select_topk(y, p, k, NINF, E.first_row), (E.tag, "enqueue_multi", q))
            for name, allow in S.tiny_masks(T.rows).items():
                dmask = _dev_u32(torch, T.pkg.row_mask(T.rows, allow))
                out = TopkOut(torch, 3, k)
                torch.cuda.synchronize()
                eng.enqueue_filtered(T.dxs.data_ptr(), 3, dmask.data_ptr(), 0, **out.ptrs())
                eng.synchronize()
                res = out.read()
                for q in range(3):
                    want = oracle.select_topk(E.ys[q], (T.present & allow).astype(np.uint8), k, NINF, E.first_row)
                    _same_topk(res["dev_idx"][q], res["dev_val"][q], want, (E.tag, "enqueue_filtered", name, q))
            ids = np.flatnonzero(T.present) + E.first_row
            val, idx = eng.similar(ids)
            for i, g in enumerate(ids):
                x = np.zeros(T.cols, dtype=np.float32)
                c, v = E.twin.get_row(int(g) - E.first_row)
                np.add.at(x, c, v)
                want = oracle.select_topk(E.layout.scores(oracle, x)[0], pres8, k, NINF, E.first_row)
                _same_topk(idx[i], val[i], want, (E.tag, "similar", int(g)))


def _check_range(T, E, boosted):
    torch = T.torch
    scores, ok = (E.sb[0], E.sb_ok[0]) if boosted else (E.ys[0], T.present)
    taus = _thresholds(scores, ok)
    kw = dict(w=T.dw, b=T.db) if boosted else dict(plain=True)
    for capacity in (0, 1, T.rows):
        got = _range(E.eng, torch, T.dx4, taus, capacity=capacity, **kw)
        for tau, (cnt, idx, val) in zip(taus, got):
            what = (E.tag, "boosted_range" if boosted else "range", tau, capacity)
            wi, wv, wn = T.pkg.boosted_matches(E.ys[0], T.present, tau, T.w if boosted else None, T.b if boosted else None, None, E.first_row)
            assert cnt == wn and idx.size == min(wn, capacity), (what, cnt, wn)
            pairs, all_pairs = set(zip(idx.tolist(), bits(val).tolist())), set(zip(wi.tolist(), bits(wv).tolist()))
            assert len(pairs) == idx.size and pairs <= all_pairs, (what, "not matches, or not distinct")
            assert capacity < wn or pairs == all_pairs, (what, "the set of (row, score bits) differs")
        assert got[0][0] == int(ok.sum()) and got[2][0] >= 1 and got[3][0] == 0, (E.tag, "-inf: all, the best score: itself, above it: none")


def _check_facets(T, E, boosted):
    scores, ok = (E.sb[0], E.sb_ok[0]) if boosted else (E.ys[0], T.present)
    taus = _thresholds(scores, ok)
    kw = dict(w=T.dw, b=T.db) if boosted else dict(plain=True)
    for n_bins in (1, 3, T.rows + 5):
        got = _facets(E.eng, T.torch, T.dx4, taus, n_bins=n_bins, labels=T.dlabels3, **kw)
        for tau, g in zip(taus, got):
            _same_facets(g, T.pkg.facet_counts(scores, ok, T.labels3, n_bins, tau, E.first_row), (E.tag, "boosted_facets" if boosted else "facets", n_bins, tau))


def test_tiny_range_and_facets(tiny):
    """enqueue_range, enqueue_boosted_range, enqueue_facets, enqueue_boosted_facets."""
    for E in tiny.engines:
        with _Counters(E.eng):
            for boosted in (False, True):
                _check_range(tiny, E, boosted)
                _check_facets(tiny, E, boosted)


def test_tiny_grouped(tiny):
    """enqueue_grouped and enqueue_boosted_grouped under three labelings."""
    T = tiny
    for E in T.engines:
        with _Counters(E.eng):
            for name, (labels, n_groups) in S.tiny_labelings(T.rows).items():
                E.eng.set_groups(labels, n_groups)
                for q, g in enumerate(_grouped(E.eng, T.torch, T.dxs, 3, plain=True)):
                    _same_grouped(g, T.pkg.collapse_topk(E.ys[q], T.present, labels, E.k, NINF, E.first_row), (E.tag, "grouped", name, q))
                for q, g in enumerate(_grouped(E.eng, T.torch, T.dxs, 3, w=T.dw, b=T.db)):
                    _same_grouped(g, T.pkg.collapse_topk(E.sb[q], E.sb_ok[q], labels, E.k, NINF, E.first_row), (E.tag, "boosted_grouped", name, q))


def _walk(T, E, boosted):
    """START to END with the device cursor chained: page p reads cursor p and writes cursor p + 1; every page is page_after's."""
    torch, eng, k = T.torch, E.eng, E.k
    scores = T.pkg.boost_scores(E.ys[0], T.minus, None) if boosted else E.ys[0]
    eligible = T.n_present
    pages = max(1, -(-eligible // k))
    assert pages <= max(1, eligible)
    out = PageOut(torch, pages, k)
    cur = support.cursors(torch, [None] * (pages + 1))
    torch.cuda.synchronize()
    for p in range(pages):
        ptrs = out.ptrs(p)
        ptrs["dev_next"] = cur.data_ptr() + 16 * (p + 1)
        if boosted:
            eng.enqueue_boosted(T.dxs.data_ptr(), 1, T.dminus.data_ptr(), 0, 0, dev_cursors=cur.data_ptr() + 16 * p, **ptrs)
        else:
            eng.enqueue_after(T.dxs.data_ptr(), 1, dev_cursors=cur.data_ptr() + 16 * p, **ptrs)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.dev["dev_next"].cpu().numpy() == -7), "dev_next went elsewhere, yet the column was written"
    out.dev["dev_next"][GUARD:GUARD + 4 * pages] = 0  # (read() checks the reserved words of the cursors)
    got = out.read()
    nxt = cur.cpu().numpy().view(np.uint32)
    assert nxt[0].tolist() == [0, 0, 0, 0], "the START cursor was written"
    cursor, seen = None, []
    for p, (idx, val, n, total, _) in enumerate(got):
        want = T.pkg.page_after(scores, T.present, k, cursor, NINF, E.first_row)
        assert nxt[p + 1, 3] == 0
        _same_page((idx, val, n, total, tuple(int(v) for v in nxt[p + 1, :3])), want, (E.tag, "boosted" if boosted else "after", "page", p))
        seen += idx[:n].tolist()
        cursor = want[4]
    assert cursor[2] == END and got[0][3] == eligible, (E.tag, "END behind the last page; the first page's total")
    assert sorted(seen) == (np.flatnonzero(T.present) + E.first_row).tolist(), (E.tag, "the union of the pages is not the eligible rows, each once")


def test_tiny_walks(tiny):
    """enqueue_after and enqueue_boosted (w = -1) from START to END."""
    for E in tiny.engines:
        with _Counters(E.eng):
            _walk(tiny, E, False)
            _walk(tiny, E, True)


def test_tiny_match_score_rows_and_row_vectors(tiny):
    T, torch, pkg, m = tiny, tiny.torch, tiny.pkg, tiny.m
    c0 = int(m.col[0])
    queries = [pkg.bool_query(T.cols, must=[c0]), pkg.bool_query(T.cols, must=[c0], must_not=[c0]), pkg.bool_query(T.cols, must=[range(T.cols)])]
    tables, preds = np.stack([t for t, _ in queries]), [p for _, p in queries]
    exp = _match_expect(pkg, m, tables, preds)
    assert exp[1][0] >= 1 and exp[1][1] == 0 and exp[1][2] == T.n_present
    for E in T.engines:
        with _Counters(E.eng):
            got = _match(torch, E.eng, tables, preds, T.rows, per_query_tables=True, out_gap=2)
            _same_match(got, exp, (E.tag, "match"), T.rows)
            # every row once, one id below first_row (where there is one), first_row + rows and the largest id
            ids = np.concatenate([np.arange(T.rows) + E.first_row, [E.first_row - 1] if E.first_row else [], [E.first_row + T.rows, OUTSIDE]]).astype(np.uint32)
            got = bits(_score_rows(torch, E.eng, T.xs, ids))
            inside = np.arange(ids.size) < T.rows
            for q in range(3):
                want = np.where(inside, np.concatenate([bits(E.ys[q]), np.zeros(ids.size - T.rows, dtype=np.uint32)]), np.uint32(NINF_BITS))
                assert np.all(bits(E.ys[q])[~T.present] == 0)
                assert np.array_equal(got[q], want), (E.tag, "score_rows", q, np.flatnonzero(got[q] != want)[:8])
            ids = np.flatnonzero(T.present) + E.first_row
            xs, ln = _run_row_vectors(torch, E.eng, ids, T.cols)
            n = ids.size
            assert np.all(bits(xs[n * T.cols:]) == bits(np.float32(-7.0))) and np.all(ln[n:] == 12345), (E.tag, "row_vectors wrote beyond its outputs")
            for i, g in enumerate(ids):
                c, v = E.twin.get_row(int(g) - E.first_row)
                want = np.zeros(T.cols, dtype=np.float32)
                np.add.at(want, c, v)
                assert ln[i] == c.size and np.array_equal(bits(xs[i * T.cols:(i + 1) * T.cols]), bits(want)), (E.tag, "row_vectors", int(g))


def test_tiny_whole_matrix_calls(tiny):
    """enqueue_row_stats, enqueue_col_stats, enqueue_assign, enqueue_nearest, enqueue_label_sums."""
    T, torch, pkg, m = tiny, tiny.torch, tiny.pkg, tiny.m
    L = pkg._lib
    for E in T.engines:
        eng = E.eng
        with _Counters(eng):
            for kind in (0, 1, 2, 3):
                out = _guarded(torch, dev_out=(T.rows, "float32"))
                torch.cuda.synchronize()
                eng.enqueue_row_stats(kind, out.ptrs()["dev_out"])
                eng.synchronize()
                assert np.array_equal(bits(out.read()["dev_out"][0]), bits(E.twin.row_stats(kind))), (E.tag, "row_stats", kind)
            for kind in (0, 1, 2):
                out = _guarded(torch, out=(T.cols, "int32"))
                torch.cuda.synchronize()
                eng.enqueue_col_stats(kind, out.ptrs()["out"])
                eng.synchronize()
                assert np.array_equal(out.read()["out"][0].view(np.uint32), pkg.col_stats(m, kind).view(np.uint32)), (E.tag, "col_stats", kind)
            for count in (1, 17):
                out = _guarded(torch, dev_labels=(T.rows, "int32"), dev_best=(T.rows, "float32"))
                torch.cuda.synchronize()
                eng.enqueue_assign(T.dnear.data_ptr(), count, **out.ptrs())
                eng.synchronize()
                res = out.read()
                wl, wb = E.twin.assign(T.near_xs[:count])
                nl, nb = pkg.nearest(E.near_y[:count])
                assert np.array_equal(wl, nl) and np.array_equal(bits(wb), bits(nb)), (E.tag, "the twin's assign against host.nearest")
                assert np.array_equal(res["dev_labels"][0].view(np.uint32), wl) and np.array_equal(bits(res["dev_best"][0]), bits(wb)), (E.tag, "assign", count)
            for count in (1, 5):
                for n in (1, 2, 3, 4):
                    out = _guarded(torch, dev_labels=(T.rows * n, "int32"), dev_scores=(T.rows * n, "float32"))
                    torch.cuda.synchronize()
                    eng.enqueue_nearest(T.dnear.data_ptr(), count, n, **out.ptrs())
                    eng.synchronize()
                    res = out.read()
                    wl, ws = E.twin.nearest(T.near_xs[:count], n)
                    gl, gs = res["dev_labels"][0].view(np.uint32).reshape(T.rows, n), res["dev_scores"][0].reshape(T.rows, n)
                    assert np.array_equal(gl, wl) and np.array_equal(bits(gs), bits(ws)), (E.tag, "nearest", count, n)
            e = eng.sums_exponent()
            assert e == E.twin.sums_exponent() == pkg.sums_exponent(m), E.tag
            for n_bins, labels in ((1, T.labels3), (3, T.labels3), (T.rows + 5, np.arange(T.rows, dtype=np.uint32))):
                want = pkg.label_sums(m, labels, n_bins, e)
                prev = np.random.default_rng(n_bins).standard_normal((n_bins, T.cols)).astype(np.float32)
                twin_sums, twin_f = E.twin.label_sums(labels, n_bins, e, L.SUMS_FLOAT)
                _, twin_u = E.twin.label_sums(labels, n_bins, e, L.SUMS_UNIT, out=prev)
                assert np.array_equal(twin_sums, want), (E.tag, "the twin's label sums")
                for flags, sink in _sinks(pkg, T.cols):
                    for mode, expect in ((L.SUMS_RAW, None), (L.SUMS_FLOAT, twin_f), (L.SUMS_UNIT, twin_u)):
                        sums, out = _sums_enqueue(pkg, torch, eng, labels, n_bins, e, mode, flags, prev if mode == L.SUMS_UNIT else None)
                        where = (E.tag, "label_sums", n_bins, sink, mode)
                        assert np.array_equal(sums, want), where
                        assert np.all(out == -7) if expect is None else np.array_equal(bits(out), bits(expect)), where
