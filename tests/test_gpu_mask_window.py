"""Allow-masks where a packet's rows span many mask words (tests/dense_ends.py), on the MI355X: every entry point that takes a mask.

mask_pair / mask_rows (kernels/packet_math.hpp) and mask_entries (kernels/col_stats.hpp) prefetch two mask words per packet and load
further ones only for a packet whose rows reach past them; nearest_kernel and nearest_fill_kernel index the mask by row. The matrices
here have packets that end hundreds of rows, packets without a row end, rows == 0, 1 and 31 mod 32, and one to three mask words
(tiny); test_mask_window_host.py asserts those properties from the packed stream.

Everything is compared exactly -- row ids, score bits, counts, mask words -- with the contract's restatements in host.py over the
order-matched oracle's scores of the engine's own layout (support.Layout), which test_mask_window_host.py pins to plain float32
arithmetic for the rows of at most two entries. Every comparison runs with clean mask words and with every bit at and beyond `rows`
set ("bits at and beyond rows are ignored", tkspmv.h): one expectation serves both. Outputs sit between guard zones, the masks
between sentinel words.

Engines (ENGINES): 4 and 8 entries per lane; first_row = 5000; a prepacked engine of two long partitions, where packets straddle rows
freely; and the three branches of launch_filtered -- deferred selection, scores + radix select (k above 3/8 of the publishing
groups), stream + select (a grid too large to defer) -- asserted from info() by create's rules as test_gpu_geometry.py restates them.
The row count plays no part in those rules, so the fixture is not repeated to reach the deferred selection. The four launch sites
of engine.hip that build a FilterParams are launch_filtered (filtered), launch_grouped (grouped, boosted_grouped), launch_after
(after, boosted) and boosted_scan (boosted_range, boosted_facets).

Evidence that the tests bite. Each mutation below was applied to a copy of the tree, the library built from it and this file run once
against it (TKSPMV_LIB); with the unchanged library every test passes.
  1. mask_rows: the further-words loop starts at `wb + 3u`. Failed: test_filtered, test_range_and_facets, test_grouped_and_after,
     test_boosted, test_boosted_forms, test_match_nearest_and_col_stats (match), test_host_forms and test_several_masks_in_one_call on
     all five engines, and test_tiny_matrices[65-4] / [65-8] (row 64 lies in the third of three mask words).
  2. mask_rows: `hi` starts at 0 (a lane whose rows begin in the packet's first mask word and cross into the second). Failed: the same
     eight functions on all five engines -- test_filtered on four of them: under c4 no affected row reaches the top 64 -- and
     test_tiny_matrices[64-8].
  3. mask_entries: `we = (rb + n_ends - 1u) >> 5` (written `rb + n_ends != 0u ? ... : 0u`, which keeps the loop bound from wrapping).
     Failed: test_match_nearest_and_col_stats (col_stats), test_host_forms (col_stats) and test_several_masks_in_one_call (col_stats;
     all layouts but stride_0, whose shared mask is random50) on the two prepacked engines ONLY: the one word this reads beyond
     mask_rows matters for a packet that ends more than two mask words of rows AND holds entries of a row that opens a mask word and
     goes on in the next packet. An engine created from so short a COO cuts partitions of one packet, where no such packet exists;
     dense_ends lays its first ordinary row out to be that row in a stream of two partitions (test_mask_window_host.py asserts it).
  4. nearest_fill_kernel ignores the mask. Failed: test_match_nearest_and_col_stats (nearest) and test_host_forms (nearest) on all
     five engines, and all twelve cases of test_tiny_matrices.
Runs 1 and 2 saw dense_ends.tiny() with rows 1, 4, 7, .. empty, under which test_tiny_matrices missed mutation 1 (row 64 was empty);
the rows 0, 3, 6, .. are empty since, and test_tiny_matrices was run against mutation 1 again (above).
The conftest syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves."""
import numpy as np
import pytest

import dense_ends
import support
from support import GuardedOut, Layout, bits
from test_gpu_boost import _query, _same as _same_page
from test_gpu_boost_forms import _facets, _grouped, _range, _same_facets, _same_grouped, _same_range
from test_gpu_match import _expect as _match_expect, _match, _same as _same_match

pytestmark = pytest.mark.gpu

END = 2
SENTINEL = 0x5EA15EA1
KINDS = (0, 1, 2)
NONE = 0xFFFFFFFF
COUNTERS = ("checks_failed", "late_repairs", "single_repairs")

NINF = float("-inf")
# name -> (rows, variant, entries per lane, k, expected branch of launch_filtered, how the engine is made). The scores are signed:
# min_score = -inf makes every allowed row with entries eligible for the ranked forms, the default 0.0 only those scoring >= 0.
ENGINES = {
    "c4": (dense_ends.ROWS[0], "last_empty", 4, 64, "deferred", dict(min_score=NINF)),
    "c8_first_row": (dense_ends.ROWS[2], "last_full", 8, 64, "deferred", dict(first_row=5000)),
    "c4_prepacked_radix": (dense_ends.ROWS[1], "last_full", 4, 400, "radix", dict(prepacked=True, min_score=NINF)),
    "c8_prepacked": (dense_ends.ROWS[2], "last_empty", 8, 64, "deferred", dict(prepacked=True)),
    "c4_stream_select": (dense_ends.ROWS[0], "last_full", 4, 64, "stream", dict(threads_per_wg=256, min_score=NINF)),
}


class TopkOut(GuardedOut):
    COLUMNS = (("dev_idx", "k", "int32"), ("dev_val", "k", "float32"))


def _path(info, k):
    """Which branch of launch_filtered serves an engine, by create's rules restated from info() (test_gpu_geometry.py: _gates, _radix)."""
    if info["n_groups"] == 0 or 8 * k > 3 * info["n_groups"]:
        return "radix"
    return "deferred" if 2 <= info["grid"] <= info["block"] + 64 else "stream"


class _Engine:
    """One engine over a dense_ends matrix with what every test needs: three query vectors and the five vectors of the nearest calls
    with the oracle's scores of the engine's own layout, labels, groups and a boost (installed, and in device memory)."""
    def __init__(self, pkg, oracle, torch, m, c_lane, k, **kw):
        self.pkg, self.torch, self.m, self.k = pkg, torch, m, k
        self.rows, self.first_row, self.min_score = m.rows, kw.get("first_row", 0), kw.get("min_score", 0.0)
        if kw.pop("prepacked", False):
            packed = pkg.Packed(m, k=k, nnz_per_lane=c_lane, n_wave_partitions=dense_ends.PREPACKED_PARTITIONS)
            self.eng = pkg.SpMV.from_packed(packed, k=k, device=0, **kw)
            assert self.eng.info()["n_wave_partitions"] == dense_ends.PREPACKED_PARTITIONS
            layout = Layout(pkg, self.eng, m, packed)
        else:
            self.eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, nnz_per_lane=c_lane, **kw)
            layout = Layout(pkg, self.eng, m)
        assert self.eng.info()["packet_entries"] == 64 * c_lane
        self.xs = np.stack([dense_ends.vector(7 + q) for q in range(3)])
        self.ys = [layout.scores(oracle, x) for x in self.xs]
        self.present = self.ys[0][1]
        assert np.array_equal(self.present, support.present(m))
        self.ys = [y for y, _ in self.ys]
        self.near_xs = np.random.default_rng(m.rows).standard_normal((5, m.cols)).astype(np.float32)
        self.near_y = np.stack([layout.scores(oracle, x)[0] for x in self.near_xs])
        r = np.arange(m.rows)
        self.labels, self.groups, self.n_groups = (r % 7).astype(np.uint32), (r // 5).astype(np.uint32), (m.rows + 4) // 5
        rng = np.random.default_rng(m.rows + 1)
        self.w, self.b = rng.uniform(0.5, 2.0, m.rows).astype(np.float32), rng.uniform(-1.0, 1.0, m.rows).astype(np.float32)
        self.sb = [pkg.boost_scores(y, self.w, self.b) for y in self.ys]
        self.eng.reset(self.xs[0])
        self.eng.set_groups(self.groups, self.n_groups)
        self.eng.set_boost(self.w, self.b)
        self.dxs = torch.from_numpy(self.xs).cuda()
        self.dnear = torch.from_numpy(self.near_xs).cuda()
        self.dlabels = torch.from_numpy(self.labels.view(np.int32)).cuda()
        self.dw, self.db = torch.from_numpy(self.w).cuda(), torch.from_numpy(self.b).cuda()
        self.clauses, self.pred = pkg.bool_query(m.cols, must=[range(0, 1000)])  # every row with an entry in a column below 1000: most rows
        ok = pkg.match_rows(m.row, m.col, m.rows, self.clauses, self.pred)
        assert m.rows < 1000 or 0.9 * self.present.sum() < ok.sum() < self.present.sum()

    def queries(self, n):
        """The device vectors of a call of n queries: vectors 0 .. n - 1."""
        return self.torch.from_numpy(np.ascontiguousarray(self.xs[:n])).cuda()

    def close(self):
        self.eng.close()


class _Masks:
    """Mask words in device memory between sentinel words: mask q at `lead` + q * stride words of the buffer (stride 0: one mask).
    check(): the sentinels and the masks themselves are what they were."""
    def __init__(self, torch, words_list, stride=0, lead=4):
        n_words = words_list[0].size
        self.host = np.full(lead + max(stride, n_words) * len(words_list) + 4, SENTINEL, dtype=np.uint32)
        for q, w in enumerate(words_list if stride else words_list[:1]):
            self.host[lead + q * stride:lead + q * stride + n_words] = w
        self.buf = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        self.dev, self.stride = self.buf[lead:], stride
        assert self.dev.data_ptr() == self.buf.data_ptr() + 4 * lead

    def check(self):
        assert np.array_equal(self.buf.cpu().numpy().view(np.uint32), self.host), "the mask buffer was written"


def _elig(E, q, allow, boosted=False, ranked=False):
    """The rows a query may return: they have entries, are allowed and (boosted) their boosted score is above -inf; ranked: the forms
    that rank rows also ask for a score of at least the engine's min_score (the threshold forms do not)."""
    s = E.sb[q] if boosted else E.ys[q]
    return E.present & allow & (s > -np.inf) & (s >= np.float32(E.min_score) if ranked else True)


def _median(v):
    return float(np.sort(v)[v.size // 2]) if v.size else 0.0


# ---- one call of each entry point: `allows` holds the mask of each query, M their words on the device ---------------------------------
def check_filtered(E, oracle, allows, M, tag):
    torch, n = E.torch, len(allows)
    out, dxs = TopkOut(torch, n, E.k), E.queries(n)
    torch.cuda.synchronize()
    E.eng.enqueue_filtered(dxs.data_ptr(), n, M.dev.data_ptr(), M.stride, **out.ptrs())
    E.eng.synchronize()
    res = out.read()
    for q, allow in enumerate(allows):
        ei, ev = oracle.select_topk(E.ys[q], _elig(E, q, allow).astype(np.uint8), E.k, E.min_score, E.first_row)
        n_real = min(E.k, int(_elig(E, q, allow, ranked=True).sum()))
        assert np.all(ei[n_real:] == 0) and np.all(bits(ev[n_real:]) == 0)  # the tail of a short list is (0, 0.0)
        assert np.array_equal(res["dev_idx"].view(np.uint32)[q], ei), (tag, q, "enqueue_filtered: row ids")
        assert np.array_equal(bits(res["dev_val"][q]), bits(ev)), (tag, q, "enqueue_filtered: score bits")
    return n


def check_range(E, allows, M, tag, boosted=False, minus_inf=False):
    """Query q at about the median eligible score of its own mask, or (minus_inf) at -inf."""
    n = len(allows)
    scores = E.sb if boosted else E.ys
    taus = [float("-inf") if minus_inf else _median(scores[q][_elig(E, q, a, boosted)]) for q, a in enumerate(allows)]
    kw = dict(w=E.dw, b=E.db) if boosted else dict(plain=True)
    got = _range(E.eng, E.torch, E.queries(n), taus, mask=M.dev, mask_stride=M.stride, rows=E.rows, **kw)
    for q, allow in enumerate(allows):
        with np.errstate(invalid="ignore"):
            hit = np.flatnonzero(_elig(E, q, allow, boosted) & (scores[q] >= np.float32(taus[q])))
        assert hit.size > 0 or not _elig(E, q, allow, boosted).any()
        _same_range(got[q], ((hit + E.first_row).astype(np.uint32), scores[q][hit], hit.size), (tag, q, taus[q]))
        if boosted:
            wi, wv, wn = E.pkg.boosted_matches(E.ys[q], E.present, taus[q], E.w, E.b, allow, E.first_row)
            _same_range(got[q], (wi, wv, wn), (tag, q, "boosted_matches"))
        if minus_inf:
            assert got[q][0] == int(_elig(E, q, allow, boosted).sum()), (tag, q, "-inf: every eligible row")


def check_facets(E, allows, M, tag, boosted=False):
    n = len(allows)
    scores = E.sb if boosted else E.ys
    taus = [_median(scores[q][_elig(E, q, a, boosted)]) for q, a in enumerate(allows)]
    kw = dict(w=E.dw, b=E.db) if boosted else dict(plain=True)
    got = _facets(E.eng, E.torch, E.queries(n), taus, n_bins=7, labels=E.dlabels, mask=M.dev, mask_stride=M.stride, **kw)
    for q, allow in enumerate(allows):
        ok = E.present & (E.sb[q] > -np.inf) if boosted else E.present
        _same_facets(got[q], E.pkg.facet_counts(scores[q], ok, E.labels, 7, taus[q], E.first_row, allow), (tag, q))


def check_grouped(E, allows, M, tag, boosted=False):
    n = len(allows)
    scores = E.sb if boosted else E.ys
    kw = dict(w=E.dw, b=E.db) if boosted else dict(plain=True)
    got = _grouped(E.eng, E.torch, E.queries(n), n, mask=M.dev, mask_stride=M.stride, **kw)
    for q, allow in enumerate(allows):
        _same_grouped(got[q], E.pkg.collapse_topk(scores[q], _elig(E, q, allow, boosted), E.groups, E.k, E.min_score, E.first_row), (tag, q))


def check_first_pages(E, allows, M, tag, boosted=False):
    """The first page of every query in one call."""
    n = len(allows)
    scores = E.sb if boosted else E.ys
    kw = dict(w=E.dw, b=E.db) if boosted else dict(after=True)
    got = _query(E.eng, E.torch, E.queries(n), n, dev_mask=M.dev.data_ptr(), mask_stride=M.stride, **kw)
    for q, allow in enumerate(allows):
        want = E.pkg.page_after(scores[q], E.present, E.k, None, E.min_score, E.first_row, allow)
        assert want[3] == int(_elig(E, q, allow, boosted, ranked=True).sum())
        _same_page(got[q], want, (tag, q))


def check_walk(E, allow, M, tag, boosted=False):
    """Query 0 paged from START to END; the first page's total is the eligible count."""
    scores, dx = (E.sb if boosted else E.ys)[0], E.queries(1)
    kw = dict(w=E.dw, b=E.db) if boosted else dict(after=True)
    cursor, seen = None, 0
    for page in range(E.rows // E.k + 2):
        got = _query(E.eng, E.torch, dx, 1, cursors=[cursor], dev_mask=M.dev.data_ptr(), mask_stride=0, **kw)[0]
        want = E.pkg.page_after(scores, E.present, E.k, cursor, E.min_score, E.first_row, allow)
        _same_page(got, want, (tag, "page", page))
        if page == 0:
            assert got[3] == int(_elig(E, 0, allow, boosted, ranked=True).sum()), (tag, "total")
        seen += got[2]
        cursor = got[4]
        if cursor[2] == END:
            break
    assert cursor[2] == END and seen == int(_elig(E, 0, allow, boosted, ranked=True).sum()), (tag, "the walk did not visit every eligible row once")


def check_match(E, allows, M, tag):
    n = len(allows)
    got = _match(E.torch, E.eng, E.clauses, [E.pred] * n, E.rows, out_gap=2, dmask=M.dev, mask_stride=M.stride)
    exp = _match_expect(E.pkg, E.m, E.clauses, [E.pred] * n, allows=list(allows))
    _same_match(got, exp, tag, E.rows)  # (words, counts, and the output's bits at and beyond rows are 0)
    for q, allow in enumerate(allows):
        assert int(exp[1][q]) == int(np.unpackbits(exp[0][q].view(np.uint8)).sum()) > (0 if allow.sum() > 40 else -1)


def check_nearest(E, allow, M, tag):
    torch = E.torch
    for n in (1, 4):
        out = type("NearestOut", (GuardedOut,), {"COLUMNS": (("dev_labels", E.rows * n, "int32"), ("dev_scores", E.rows * n, "float32"))})(torch, 1, 0)
        torch.cuda.synchronize()
        E.eng.enqueue_nearest(E.dnear.data_ptr(), 5, n, dev_mask=M.dev.data_ptr(), **out.ptrs())
        E.eng.synchronize()
        res = out.read()
        gl, gs = res["dev_labels"].view(np.uint32).reshape(E.rows, n), res["dev_scores"].reshape(E.rows, n)
        wl, ws = E.pkg.nearest_n(E.near_y, n, allow)
        assert np.all(gl[~allow] == NONE) and np.all(np.isneginf(gs[~allow])), (tag, n, "a row outside the mask is not (NONE, -inf) throughout")
        assert np.array_equal(gl, wl) and np.array_equal(bits(gs), bits(ws)), (tag, n, "enqueue_nearest differs from nearest_n")


def check_col_stats(E, allows, M, tag):
    torch, n, cols = E.torch, len(allows), E.m.cols
    total = np.bincount(E.m.row, minlength=E.rows)
    for kind in KINDS:
        out = type("ColOut", (GuardedOut,), {"COLUMNS": (("out", cols + 3, "int32"),)})(torch, n, 0)
        torch.cuda.synchronize()
        E.eng.enqueue_col_stats(kind, out.ptrs()["out"], masks=M.dev.data_ptr(), mask_stride=M.stride, out_stride=cols + 3, count=n)
        E.eng.synchronize()
        got = out.read()["out"].view(np.uint32)
        assert np.all(got[:, cols:] == np.uint32(0xFFFFFFF9)), (tag, kind, "the words between the sets were written")
        for q, allow in enumerate(allows):
            assert np.array_equal(got[q, :cols], E.pkg.col_stats(E.m, kind, allow).view(np.uint32)), (tag, kind, q, "enqueue_col_stats differs from col_stats")
            if kind == 0:  # no padding and no placeholder is counted
                assert int(got[q, :cols].sum()) == int(total[allow].sum()), (tag, q, "COL_NNZ does not sum to the entries of the allowed rows")


def check_host_forms(E, oracle, allow, w, tag):
    """The run_* / use_filter forms with the mask installed from host words w: query 0, the installed groups and boost."""
    pkg, eng, y, sb, k, fr, ms = E.pkg, E.eng, E.ys[0], E.sb[0], E.k, E.first_row, E.min_score
    eng.reset(E.xs[0])
    val, idx = eng.run_filtered(allow=w)
    ei, ev = oracle.select_topk(y, _elig(E, 0, allow).astype(np.uint8), k, ms, fr)
    assert np.array_equal(idx, ei) and np.array_equal(bits(val), bits(ev)), (tag, "run_filtered")
    t = _median(y[_elig(E, 0, allow)])
    rv, ri = eng.run_range(t, allow=w)
    wi, wv, wn = pkg.boosted_matches(y, E.present, t, None, None, allow, fr)  # (no boost: run_range's set in run_range's order)
    assert eng.last_range_count == wn and np.array_equal(ri, wi) and np.array_equal(bits(rv), bits(wv)), (tag, "run_range")
    _same_facets(eng.run_facets(t, allow=w), pkg.facet_counts(y, E.present, E.groups, E.n_groups, t, fr, allow), (tag, "run_facets"))
    gv, gi, gg = eng.run_grouped(allow=w)
    ci, cv, cg, cn = pkg.collapse_topk(y, _elig(E, 0, allow), E.groups, k, ms, fr)
    assert gi.size == cn and np.array_equal(gi, ci[:cn]) and np.array_equal(bits(gv), bits(cv[:cn])) and np.array_equal(gg, cg[:cn]), (tag, "run_grouped")
    _same_page(eng.run_after(None, allow=w), pkg.page_after(y, E.present, k, None, ms, fr, allow), (tag, "run_after"))
    _same_page(eng.run_boosted(None, allow=w), pkg.page_after(sb, E.present, k, None, ms, fr, allow), (tag, "run_boosted"))
    tb = _median(sb[_elig(E, 0, allow, True)])
    rv, ri = eng.run_boosted_range(tb, allow=w)
    wi, wv, wn = pkg.boosted_matches(y, E.present, tb, E.w, E.b, allow, fr)
    assert eng.last_range_count == wn and np.array_equal(ri, wi) and np.array_equal(bits(rv), bits(wv)), (tag, "run_boosted_range")
    _same_facets(eng.run_boosted_facets(tb, allow=w), pkg.facet_counts(sb, E.present & (sb > -np.inf), E.groups, E.n_groups, tb, fr, allow),
                 (tag, "run_boosted_facets"))
    gv, gi, gg = eng.run_boosted_grouped(allow=w)
    ci, cv, cg, cn = pkg.collapse_topk(sb, _elig(E, 0, allow, True), E.groups, k, ms, fr)
    assert gi.size == cn and np.array_equal(gi, ci[:cn]) and np.array_equal(bits(gv), bits(cv[:cn])) and np.array_equal(gg, cg[:cn]), (tag, "run_boosted_grouped")
    words, count = eng.match(E.clauses, E.pred, allow=w)
    ok = pkg.match_rows(E.m.row, E.m.col, E.rows, E.clauses, E.pred, allow=allow)
    assert count == int(ok.sum()) and np.array_equal(words, pkg.row_mask(E.rows, ok)), (tag, "match")
    for n in (1, 4):
        gl, gs = eng.nearest(E.near_xs, n, mask=w)
        wl, ws = pkg.nearest_n(E.near_y, n, allow)
        assert np.array_equal(gl, wl) and np.array_equal(bits(gs), bits(ws)), (tag, "nearest", n)
    for kind in KINDS:
        assert np.array_equal(eng.col_stats(kind, use_filter=True).view(np.uint32), pkg.col_stats(E.m, kind, allow).view(np.uint32)), (tag, "col_stats", kind)


# ---- the engines ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(pkg, oracle):
    import torch
    made = {}

    def get(name):
        if name not in made:
            rows, variant, c_lane, k, _, kw = ENGINES[name]
            made[name] = _Engine(pkg, oracle, torch, dense_ends.matrix(pkg, rows, variant), c_lane, k, **kw)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _every_mask(E):
    """(name, allow, dirty, words on the device) of every mask of the fixture, clean and dirty."""
    for name, allow in dense_ends.masks(E.rows).items():
        for dirty in (False, True):
            M = _Masks(E.torch, [dense_ends.words(E.pkg, E.rows, allow, dirty)])
            yield f"{name}/{'dirty' if dirty else 'clean'}", allow, M
            M.check()


@pytest.mark.parametrize("name", list(ENGINES))
def test_engine_paths(engines, name):
    """Which branch of launch_filtered each engine is on, from info() by create's rules; between them the engines cover all three."""
    E = engines(name)
    info = E.eng.info()
    assert _path(info, E.k) == ENGINES[name][4], info
    assert {v[4] for v in ENGINES.values()} == {"deferred", "radix", "stream"}
    assert {v[2] for v in ENGINES.values()} == {4, 8} and any(v[5].get("first_row") for v in ENGINES.values())


@pytest.mark.parametrize("name", list(ENGINES))
def test_filtered(engines, oracle, name):
    E = engines(name)
    small = 0
    for tag, allow, M in _every_mask(E):
        check_filtered(E, oracle, [allow], M, f"{name}/{tag}")
        small += int(_elig(E, 0, allow, ranked=True).sum()) > E.k
    assert 0 < small < 2 * len(dense_ends.masks(E.rows))  # k below the eligible count under some masks, above it under others


@pytest.mark.parametrize("name", list(ENGINES))
def test_range_and_facets(engines, name):
    E = engines(name)
    c0 = E.eng.debug_counters()
    for tag, allow, M in _every_mask(E):
        check_range(E, [allow], M, f"{name}/range/{tag}")
        check_range(E, [allow], M, f"{name}/range -inf/{tag}", minus_inf=True)
        check_facets(E, [allow], M, f"{name}/facets/{tag}")
    c1 = E.eng.debug_counters()
    assert all(c0[c] == c1[c] for c in COUNTERS), (c0, c1)


@pytest.mark.parametrize("name", list(ENGINES))
def test_grouped_and_after(engines, name):
    E = engines(name)
    for tag, allow, M in _every_mask(E):
        check_grouped(E, [allow], M, f"{name}/grouped/{tag}")
        check_walk(E, allow, M, f"{name}/after/{tag}")


@pytest.mark.parametrize("name", list(ENGINES))
def test_boosted(engines, name):
    E = engines(name)
    for tag, allow, M in _every_mask(E):
        check_walk(E, allow, M, f"{name}/boosted/{tag}", boosted=True)


@pytest.mark.parametrize("name", list(ENGINES))
def test_boosted_forms(engines, name):
    E = engines(name)
    for tag, allow, M in _every_mask(E):
        check_range(E, [allow], M, f"{name}/boosted_range/{tag}", boosted=True)
        check_range(E, [allow], M, f"{name}/boosted_range -inf/{tag}", boosted=True, minus_inf=True)
        check_facets(E, [allow], M, f"{name}/boosted_facets/{tag}", boosted=True)
        check_grouped(E, [allow], M, f"{name}/boosted_grouped/{tag}", boosted=True)


@pytest.mark.parametrize("name", list(ENGINES))
def test_match_nearest_and_col_stats(engines, name):
    E = engines(name)
    c0 = E.eng.debug_counters()
    for tag, allow, M in _every_mask(E):
        check_match(E, [allow], M, f"{name}/match/{tag}")
        check_nearest(E, allow, M, f"{name}/nearest/{tag}")
        check_col_stats(E, [allow], M, f"{name}/col_stats/{tag}")
    c1 = E.eng.debug_counters()
    assert all(c0[c] == c1[c] for c in COUNTERS), (c0, c1)


@pytest.mark.parametrize("name", list(ENGINES))
def test_host_forms(engines, oracle, name):
    E = engines(name)
    for mname, allow in dense_ends.masks(E.rows).items():
        for dirty in (False, True):
            check_host_forms(E, oracle, allow, dense_ends.words(E.pkg, E.rows, allow, dirty), f"{name}/{mname}/{'dirty' if dirty else 'clean'}")
    E.eng.set_filter(None)


@pytest.mark.parametrize("layout", ["stride_words", "stride_words_plus_3", "stride_0", "unaligned"])
@pytest.mark.parametrize("name", list(ENGINES))
def test_several_masks_in_one_call(engines, oracle, name, layout):
    """Three queries, each with another vector and another mask (dirty words): masks back to back; three sentinel words between them;
    one mask for all (stride 0); and a mask pointer that is 4-byte but not 16-byte aligned, with an odd stride."""
    E = engines(name)
    masks = dense_ends.masks(E.rows)
    allows = [masks["random50"], masks["alt_words"], masks["word_edges"]]
    words = [dense_ends.words(E.pkg, E.rows, a, True) for a in allows]
    n_words = words[0].size
    stride, lead = {"stride_words": (n_words, 4), "stride_words_plus_3": (n_words + 3, 4), "stride_0": (0, 4), "unaligned": (n_words + 3, 5)}[layout]
    if stride == 0:
        allows = allows[:1] * 3
    M = _Masks(E.torch, words, stride, lead)
    assert M.dev.data_ptr() % 16 == (4 if layout == "unaligned" else 0)
    tag = f"{name}/{layout}"
    c0 = E.eng.debug_counters()
    check_range(E, allows, M, tag + "/range")
    check_facets(E, allows, M, tag + "/facets")
    check_match(E, allows, M, tag + "/match")
    check_col_stats(E, allows, M, tag + "/col_stats")
    c1 = E.eng.debug_counters()
    assert all(c0[c] == c1[c] for c in COUNTERS), (c0, c1)
    check_filtered(E, oracle, allows, M, tag + "/filtered")
    check_grouped(E, allows, M, tag + "/grouped")
    check_first_pages(E, allows, M, tag + "/after")
    check_first_pages(E, allows, M, tag + "/boosted", boosted=True)
    check_range(E, allows, M, tag + "/boosted_range", boosted=True)
    check_facets(E, allows, M, tag + "/boosted_facets", boosted=True)
    check_grouped(E, allows, M, tag + "/boosted_grouped", boosted=True)
    M.check()


# ---- masks of one, two and three words --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_lane", [4, 8])
@pytest.mark.parametrize("rows", dense_ends.TINY_ROWS)
def test_tiny_matrices(pkg, oracle, rows, c_lane):
    """1 .. 65 rows: F.words - 1 == 0, and w + 1 clamped from the first packet on. Filtered, range, facets, nearest and col_stats under
    the even-rows and odd-rows masks, clean and dirty."""
    import torch
    E = _Engine(pkg, oracle, torch, dense_ends.tiny(pkg, rows), c_lane, 4, min_score=NINF)
    assert pkg.row_mask(rows, None).size == (rows + 31) // 32 <= 3
    c0 = E.eng.debug_counters()
    for mname, allow in dense_ends.tiny_masks(rows).items():
        for dirty in (False, True):
            M = _Masks(torch, [dense_ends.words(pkg, rows, allow, dirty)])
            tag = f"tiny {rows}/C={c_lane}/{mname}/{'dirty' if dirty else 'clean'}"
            check_filtered(E, oracle, [allow], M, tag)
            check_range(E, [allow], M, tag + "/range")
            check_range(E, [allow], M, tag + "/range -inf", minus_inf=True)
            check_facets(E, [allow], M, tag + "/facets")
            check_nearest(E, allow, M, tag + "/nearest")
            check_col_stats(E, [allow], M, tag + "/col_stats")
            M.check()
    c1 = E.eng.debug_counters()
    assert all(c0[c] == c1[c] for c in COUNTERS), (c0, c1)
    E.close()
