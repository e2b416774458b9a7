"""Boolean term predicates (tkspmv_enqueue_match / tkspmv_run_match) on the MI355X.

The expectation is match_rows -- the contract restated in numpy from the COO alone, itself checked against a plain loop in
test_match_host.py -- packed with row_mask: the device mask must equal it word for word and dev_counts its popcount. Output buffers
carry a pattern around and between the masks, which must survive. The conftest syncs torch only for the older enqueue names: these
tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import bits

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A


def _dev(torch, a):
    a = np.array(a)  # (a contiguous, writable copy: torch wants one)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _pred_array(preds):
    return np.array([[int(v) & 0xFFFFFFFF for v in p] for p in preds], dtype=np.uint32)


def _match(torch, eng, tables, preds, rows, per_query_tables=False, out_gap=0, counts=True, dmask=None, mask_stride=0, stream=None, wait=True):
    """One enqueue_match call into pattern-filled buffers: a guard word in front of dev_out and of dev_counts, out_gap words between
    the masks and behind the last one (at least one). Returns read() -> (masks[nq, words], counts[nq] or None), which checks that
    every word outside the masks still holds the pattern; wait=False: nothing is waited for behind the call."""
    nq, words = len(preds), max(1, (rows + 31) // 32)
    stride = words + out_gap
    dt = _dev(torch, np.ascontiguousarray(tables, dtype=np.uint32).ravel())
    dp = _dev(torch, _pred_array(preds).ravel())
    do = _dev(torch, np.full(1 + nq * stride + 1, FILL, dtype=np.uint32))
    dc = _dev(torch, np.full(nq + 2, FILL, dtype=np.uint32)) if counts else None
    torch.cuda.synchronize()
    cols = eng.num_cols
    eng.enqueue_match(dt.data_ptr(), dp.data_ptr(), nq, do.data_ptr() + 4, out_stride=stride if (nq > 1 or out_gap) else 0,
                      dev_counts=dc.data_ptr() + 4 if counts else 0, clause_stride=cols if per_query_tables else 0,
                      dev_mask=dmask.data_ptr() if dmask is not None else 0, mask_stride=mask_stride,
                      stream=stream.cuda_stream if stream is not None else 0)
    keep = (dt, dp, dmask)

    def read():
        assert keep
        ho = do.cpu().numpy().view(np.uint32)
        assert ho[0] == FILL and ho[-1] == FILL, "dev_out was written outside the masks"
        body = ho[1:-1].reshape(nq, stride)
        assert np.all(body[:, words:] == FILL), "the words between the masks of a strided output were written"
        hc = None
        if counts:
            hc = dc.cpu().numpy().view(np.uint32)
            assert hc[0] == FILL and hc[-1] == FILL, "dev_counts was written outside count entries"
            hc = hc[1:-1].copy()
        return body[:, :words].copy(), hc
    if not wait:
        return read
    if stream is not None:
        stream.synchronize()
    else:
        eng.synchronize()
    torch.cuda.synchronize()
    return read()


def _expect(pkg, m, tables, preds, allows=None):
    """row_mask(match_rows) per query; tables [cols] (one for all) or [nq, cols]; allows None, one bool array or a list per query."""
    tables = np.asarray(tables, dtype=np.uint32)
    masks, counts = [], []
    for i, p in enumerate(preds):
        t = tables if tables.ndim == 1 else tables[i]
        allow = None if allows is None else (allows[i] if isinstance(allows, list) else allows)
        ok = pkg.match_rows(m.row, m.col, m.rows, t, p, allow=allow)
        masks.append(pkg.row_mask(m.rows, ok))
        counts.append(int(ok.sum()))
    return np.stack(masks), np.array(counts, dtype=np.uint32)


def _same(got, exp, label, rows):
    (gm, gc), (em, ec) = got, exp
    bad = np.argwhere(gm != em)
    assert bad.size == 0, f"{label}: {len(bad)} mask words differ, first query {bad[0][0]} word {bad[0][1]}: {gm[tuple(bad[0])]:#010x} != {em[tuple(bad[0])]:#010x}"
    if rows % 32:
        assert not np.any(gm[:, -1] >> np.uint32(rows % 32)), f"{label}: bits at and beyond rows are set"
    if gc is not None:
        assert np.array_equal(gc, ec), f"{label}: counts {gc.tolist()} != {ec.tolist()}"


def _popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


# ---- the twelve predicates of a generated matrix: one shared table, columns chosen by frequency ------------------------------------
def _twelve(m):
    """(table uint32[cols], [12 predicates]). Clause bits: 0 a rare column, 1 the most frequent column, 2-4 three frequent columns,
    5 the banned columns, 6-8 three sets of columns, 31 a set of its own; one column belongs to all 32 clauses."""
    freq = np.bincount(m.col, minlength=m.cols)
    order = np.argsort(freq, kind="stable")
    used = order[freq[order] > 0]
    rare, top = int(used[0]), int(order[-1])
    t = np.zeros(m.cols, dtype=np.uint32)
    t[rare] |= 1 << 0
    t[top] |= 1 << 1
    for b, c in zip((2, 3, 4), order[-4:-1]):
        t[int(c)] |= 1 << b
    rng = np.random.default_rng(m.cols + m.rows)
    pool = rng.permutation(order[: max(8, m.cols - 8)])
    w = max(2, m.cols // 10)
    t[pool[0:8]] |= 1 << 5
    for b in (6, 7, 8):
        t[pool[8 + (b - 6) * w: 8 + (b - 5) * w]] |= 1 << b
    t[pool[8 + 3 * w: 8 + 3 * w + max(2, w // 4)]] |= np.uint32(1 << 31)
    t[int(used[len(used) // 2])] = 0xFFFFFFFF
    sh = (1 << 6) | (1 << 7) | (1 << 8)
    preds = [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (0b11100, 0, 0, 0), (0, 1 << 5, 0, 0),
             (0, 0, sh, 1), (0, 0, sh, 2), (0, 0, sh, 3), (0, 0, sh, 4), (1 << 31, 0, 0, 0), (0xFFFFFFFF, 0, 0, 0),
             (2, 1 << 5, sh, 1)]
    return t, preds


SHAPES = [
    (1000, 512, {}),
    (50_000, 1024, {}),
    (50_000, 1024, {"nnz_per_lane": 8}),
    (20_000, 4096, {}),
    (8000, 16384, {}),
    (200_000, 1024, {}),
]
IDS = ["1000x512", "50kx1024", "c8", "20kx4096", "8kx16384", "200kx1024"]


class _Case:
    def __init__(self, pkg, rows, cols, kw):
        self.m = pkg.generate_matrix(rows, cols, 20, "gamma", rows % 89 + 5)
        self.eng = pkg.SpMV(self.m.row, self.m.col, self.m.val, rows, cols, k=100, device=0, **kw)
        self.table, self.preds = _twelve(self.m)
        self.exp = _expect(pkg, self.m, self.table, self.preds)  # computed once, shared, never changed
        self.exp[0].setflags(write=False)
        self.exp[1].setflags(write=False)


@pytest.fixture(scope="module")
def cases(pkg):
    made = {}

    def get(i):
        if i not in made:
            made[i] = _Case(pkg, *SHAPES[i])
        return made[i]
    yield get
    for c in made.values():
        c.eng.close()


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=IDS)
def test_twelve_predicates(pkg, cases, shape):
    """The twelve predicates in one call over one table (stride 0), with gaps of 3 words between the masks; again with one table per
    query (stride cols), densely; the counts run from 0 to nearly every row."""
    import torch
    c = cases(shape)
    rows = c.m.rows
    present = int(np.unique(c.m.row).size)
    ec = c.exp[1]
    assert ec[0] == present and ec[8] == 0 and ec.max() == present and np.count_nonzero(ec) >= 8, ec.tolist()
    assert ec[4] > 0.5 * present and 0 < ec[1] < 0.2 * present, ec.tolist()
    _same(_match(torch, c.eng, c.table, c.preds, rows, out_gap=3), c.exp, f"{IDS[shape]}/shared", rows)
    tables = np.stack([np.roll(c.table, 7 * i) for i in range(12)])
    exp = _expect(pkg, c.m, tables, c.preds)
    _same(_match(torch, c.eng, tables, c.preds, rows, per_query_tables=True), exp, f"{IDS[shape]}/per_query", rows)
    # without dev_counts, and a single query with out_stride 0
    gm, gc = _match(torch, c.eng, c.table, c.preds, rows, counts=False)
    assert gc is None
    _same((gm, None), c.exp, f"{IDS[shape]}/no_counts", rows)
    one = _match(torch, c.eng, c.table, c.preds[11:], rows)
    _same(one, (c.exp[0][11:], c.exp[1][11:]), f"{IDS[shape]}/single", rows)


@pytest.mark.parametrize("shape", [1, 2, 5], ids=[IDS[1], IDS[2], IDS[5]])
def test_with_allow_mask(pkg, cases, shape):
    """The result is predicate AND mask: the 50 % and the 0.1 % random masks for every query, and one mask per query."""
    import torch
    c = cases(shape)
    rows = c.m.rows
    rng = np.random.default_rng(rows + 1)
    allows = {d: rng.random(rows) < d for d in (0.5, 0.001)}
    for d, allow in allows.items():
        dmask = _dev(torch, pkg.row_mask(rows, allow))
        exp = _expect(pkg, c.m, c.table, c.preds, allow)
        assert np.array_equal(exp[0], c.exp[0] & pkg.row_mask(rows, allow)[None, :])
        _same(_match(torch, c.eng, c.table, c.preds, rows, dmask=dmask), exp, f"{IDS[shape]}/allow{d}", rows)
    per_q = [allows[0.5] if i % 2 else allows[0.001] for i in range(12)]
    words = np.stack([pkg.row_mask(rows, a) for a in per_q])
    exp = _expect(pkg, c.m, c.table, c.preds, per_q)
    _same(_match(torch, c.eng, c.table, c.preds, rows, dmask=_dev(torch, words), mask_stride=words.shape[1], out_gap=1), exp,
          f"{IDS[shape]}/allow_per_query", rows)


def test_forty_predicates_cross_the_launch_boundary(pkg, cases):
    import torch
    c = cases(0)
    rng = np.random.default_rng(40)
    preds = [c.preds[i % 12] for i in range(40)]
    tables = np.stack([np.roll(c.table, int(s)) for s in rng.integers(0, c.m.cols, 40)])
    exp = _expect(pkg, c.m, tables, preds)
    assert len({int(x) for x in exp[1]}) > 10
    _same(_match(torch, c.eng, tables, preds, c.m.rows, per_query_tables=True, out_gap=2), exp, "forty", c.m.rows)
    _same(_match(torch, c.eng, c.table, preds, c.m.rows), _expect(pkg, c.m, c.table, preds), "forty/shared", c.m.rows)


# ---- the hand-built matrix ---------------------------------------------------------------------------------------------------------
E_ROWS, E_COLS = 2085, 1024


def _edges(pkg, last_row_empty):
    """2085 rows x 1024 columns. Clause-bearing columns: 0, 1023, 950, 951, 952, 953 and the sets the table names; ordinary entries
    use columns 100..899."""
    rng = np.random.default_rng(2085)
    ent = {}  # row -> [(col, val)] in the order given

    def ordinary(n):
        return [(int(c), float(v)) for c, v in zip(rng.choice(np.arange(100, 900), n, replace=False), rng.random(n) + 0.1)]
    for r in range(1, 100):                      # row 0 stays empty
        ent[r] = ordinary(int(rng.integers(1, 30)))
        if r % 7 == 0:
            ent[r].append((int(rng.choice([0, 1023, 950, 952, 10, 40, 960, 970, 980])), 0.5))
    # rows 100..139: 40 empty rows
    for r in range(140, 200):                    # one entry each
        ent[r] = [(int(rng.choice([0, 1023, 5, 10, 40, 300, 952, 953, 960, 970, 980])), 1.0)]
    ent[200] = [(0, 0.25)] + [(c, 0.5) for c in range(100, 799)]          # 700 entries, the only clause-bearing column in the first
    ent[201] = [(c, 0.5) for c in range(100, 799)] + [(1023, 0.25)]       # ... and in the last
    ent[202] = [(950, 0.5), (950, 0.25), (105, 1.0)]                      # a repeated column
    ent[203] = [(951, 0.0), (107, 1.0)]                                   # the only clause-bearing entry has value 0.0
    for r in range(204, 300):
        if r % 5:
            ent[r] = ordinary(int(rng.integers(1, 12)))
    for r in range(300, 400):                    # negative values throughout
        ent[r] = [(c, -v) for c, v in ordinary(int(rng.integers(1, 40)))] + ([(960, -1.0)] if r % 3 == 0 else []) + ([(40, -0.5)] if r % 4 == 0 else [])
    for r in range(400, E_ROWS):
        if r % 11 == 0:
            continue
        ent[r] = ordinary(int(rng.integers(1, 25)))
        pick = rng.random()
        if pick < 0.3:
            ent[r].append((int(rng.choice([10, 20, 30, 960, 961, 970, 971, 980, 981, 952, 953])), 0.75))
        if pick < 0.1:
            ent[r].append((int(rng.choice([40, 45, 60, 0, 1023])), 0.75))
        if pick < 0.15:
            ent[r].append((int(rng.choice([965, 975, 985])), 0.5))
    if last_row_empty:
        ent.pop(E_ROWS - 1, None)
    else:
        ent[E_ROWS - 1] = [(1023, 1.0), (200, 1.0)]
    row, col, val = [], [], []
    for r in sorted(ent):
        for c, v in ent[r]:
            row.append(r)
            col.append(c)
            val.append(v)
    m = pkg.CooMatrix(rows=E_ROWS, cols=E_COLS, row=np.array(row, dtype=np.uint32), col=np.array(col, dtype=np.uint32), val=np.array(val, dtype=np.float32))
    t = np.zeros(E_COLS, dtype=np.uint32)
    t[0], t[1023], t[950], t[951] = 1 << 0, 1 << 1, 1 << 2, 1 << 3
    t[[10, 20, 30]] = 1 << 4
    t[40:61] = 1 << 5
    t[960:970], t[970:980], t[980:990] = 1 << 6, 1 << 7, 1 << 8
    t[952] = np.uint32(1 << 31)
    t[953] = 0xFFFFFFFF
    sh = (1 << 6) | (1 << 7) | (1 << 8)
    preds = [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (4, 0, 0, 0), (8, 0, 0, 0), (3, 0, 0, 0), (0, 1 << 5, 0, 0), (0, 0, sh, 1), (0, 0, sh, 2),
             (0, 0, sh, 3), (0, 0, sh, 4), (1 << 31, 0, 0, 0), (0xFFFFFFFF, 0, 0, 0), (1 << 4, 1 << 5, sh, 1), (0, 1 | 2, 1 << 4, 0)]
    return m, t, preds


@pytest.mark.parametrize("nnz_per_lane", [4, 8])
@pytest.mark.parametrize("last_row_empty", [True, False], ids=["last_empty", "last_full"])
def test_edges(pkg, nnz_per_lane, last_row_empty):
    import torch
    m, t, preds = _edges(pkg, last_row_empty)
    exp = _expect(pkg, m, t, preds)
    ok = lambda i: set(np.flatnonzero(pkg.match_rows(m.row, m.col, m.rows, t, preds[i])).tolist())
    # the rows the matrix was built for are where the expectation says
    assert 0 not in ok(0) and not (ok(0) & set(range(100, 140))) and ((E_ROWS - 1) in ok(0)) == (not last_row_empty)
    assert 200 in ok(1) and 201 not in ok(1) and 201 in ok(2) and 200 not in ok(2)
    assert 202 in ok(3) and 203 in ok(4) and 200 not in ok(5) and 201 not in ok(5)
    assert {r for r in range(300, 400) if r % 3 == 0} <= ok(7)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, nnz_per_lane=nnz_per_lane)
    try:
        assert eng.info()["packet_entries"] == 64 * nnz_per_lane
        _same(_match(torch, eng, t, preds, m.rows, out_gap=3), exp, "edges/shared", m.rows)
        tables = np.stack([t] * len(preds))
        _same(_match(torch, eng, tables, preds, m.rows, per_query_tables=True), exp, "edges/per_query", m.rows)
        allow = np.random.default_rng(3).random(m.rows) < 0.5
        _same(_match(torch, eng, t, preds, m.rows, dmask=_dev(torch, pkg.row_mask(m.rows, allow))), _expect(pkg, m, t, preds, allow), "edges/allow", m.rows)
        # the host form, with and without the count and the mask
        for i in (0, 1, 6, 13):
            words, count = eng.match(t, preds[i])
            assert np.array_equal(words, exp[0][i]) and count == exp[1][i], i
    finally:
        eng.close()


# ---- composition -------------------------------------------------------------------------------------------------------------------
def test_feeds_filtered_range_and_facets_unwaited(pkg, cases):
    """enqueue_match directly followed, on the engine's stream and with nothing waited for, by enqueue_filtered, enqueue_range and
    enqueue_facets reading its output: the same as those calls given the mask the host built."""
    import torch
    c = cases(1)
    eng, m = c.eng, c.m
    rows, words, k = m.rows, (m.rows + 31) // 32, eng.k
    x = np.ascontiguousarray(pkg.create_sample_vector(m.cols, True, False, True, 9), dtype=np.float32)
    dx = _dev(torch, x)
    pred = c.preds[5]
    host_words = c.exp[0][5]
    lab = (np.arange(rows) % 16).astype(np.uint32)
    dlab, dthr = _dev(torch, lab), _dev(torch, np.array([0.0], dtype=np.float32))

    def run(dmask_ptr, before):
        oi = torch.zeros((k,), dtype=torch.int32, device="cuda")
        ov = torch.zeros((k,), dtype=torch.float32, device="cuda")
        rc = torch.zeros((1,), dtype=torch.int32, device="cuda")
        ri = torch.zeros((rows,), dtype=torch.int32, device="cuda")
        rv = torch.zeros((rows,), dtype=torch.float32, device="cuda")
        fc = torch.zeros((16,), dtype=torch.int32, device="cuda")
        fb = torch.zeros((16,), dtype=torch.int64, device="cuda")
        ft = torch.zeros((1,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        before()
        eng.enqueue_filtered(dx.data_ptr(), 1, dmask_ptr, 0, oi.data_ptr(), ov.data_ptr())
        eng.enqueue_range(dx.data_ptr(), 1, dthr.data_ptr(), rc.data_ptr(), ri.data_ptr(), rv.data_ptr(), rows, dmask_ptr)
        eng.enqueue_facets(dx.data_ptr(), 1, dthr.data_ptr(), fc.data_ptr(), 16, dlab.data_ptr(), fb.data_ptr(), ft.data_ptr(), dmask_ptr)
        eng.synchronize()
        torch.cuda.synchronize()
        n = int(rc.cpu().numpy().view(np.uint32)[0])
        hi, hv = ri.cpu().numpy().view(np.uint32)[:n], bits(rv.cpu().numpy()[:n])
        o = np.lexsort((hv, hi))  # (range results come in no particular order)
        return (oi.cpu().numpy().view(np.uint32), bits(ov.cpu().numpy()), n, hi[o], hv[o], fc.cpu().numpy().view(np.uint32),
                fb.cpu().numpy(), ft.cpu().numpy().view(np.uint32))

    dhost = _dev(torch, host_words)
    ref = run(dhost.data_ptr(), lambda: None)
    dt, dp = _dev(torch, c.table), _dev(torch, _pred_array([pred]).ravel())
    dout = _dev(torch, np.full(words, FILL, dtype=np.uint32))
    got = run(dout.data_ptr(), lambda: eng.enqueue_match(dt.data_ptr(), dp.data_ptr(), 1, dout.data_ptr()))
    assert np.array_equal(dout.cpu().numpy().view(np.uint32), host_words)
    assert 0 < ref[2] <= int(c.exp[1][5]) and ref[7][0] == ref[2]
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_run_match_installs_the_filter(pkg, cases):
    """tkspmv_run_match(install=1) then run_filtered equals run_filtered with the host mask; with use_filter as well the installed
    filter is the old one AND the predicate."""
    c = cases(1)
    eng, m = c.eng, c.m
    x = pkg.create_sample_vector(m.cols, True, False, True, 4)
    ok = pkg.match_rows(m.row, m.col, m.rows, c.table, c.preds[5])
    try:
        ev, ei = eng.run_filtered(vec=x, allow=ok)
        eng.set_filter(None)
        words, count = eng.match(c.table, c.preds[5], install=True)
        assert np.array_equal(words, c.exp[0][5]) and count == c.exp[1][5]
        eng.enqueue_filtered(0, 1, 0)
        eng.synchronize()
        gv, gi = eng.read_result()
        assert np.array_equal(gi, ei) and np.array_equal(bits(gv), bits(ev))
        # AND with the installed filter
        allow = np.random.default_rng(8).random(m.rows) < 0.5
        both = ok & allow
        ev, ei = eng.run_filtered(vec=x, allow=both)
        words, count = eng.match(c.table, c.preds[5], allow=allow, install=True)
        assert np.array_equal(words, pkg.row_mask(m.rows, both)) and count == int(both.sum())
        eng.enqueue_filtered(0, 1, 0)
        eng.synchronize()
        gv, gi = eng.read_result()
        assert np.array_equal(gi, ei) and np.array_equal(bits(gv), bits(ev))
        # host_mask and count may each be NULL; use_filter with none installed is an error
        lib = pkg._lib.lib()
        rec = pkg._lib.Match(*c.preds[5])
        tab = np.ascontiguousarray(c.table)
        assert lib.tkspmv_run_match(eng._h, tab.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rec), 0, 0, None, None) == pkg._lib.OK
        eng.set_filter(None)
        assert lib.tkspmv_run_match(eng._h, tab.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rec), 1, 0, None, None) == pkg._lib.ERR_INVALID
    finally:
        eng.set_filter(None)


def test_no_cross_talk_with_the_batch(pkg, cases):
    """enqueue_match directly behind enqueue_batch on the engine's stream, unwaited: the batch's lists are what a fresh engine gives
    without it."""
    import torch
    c = cases(1)
    m = c.m
    nq, k = 8, 100
    xs = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 700 + i) for i in range(nq)]).astype(np.float32)
    dxs = _dev(torch, xs)

    def batch(then):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
        try:
            oi = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
            ov = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.enqueue_batch(dxs.data_ptr(), nq, oi.data_ptr(), ov.data_ptr())
            read = then(eng)  # (not waited for: right behind the batch launch)
            eng.synchronize()
            torch.cuda.synchronize()
            return oi.cpu().numpy().view(np.uint32).copy(), bits(ov.cpu().numpy()).copy(), read() if read else None
        finally:
            eng.close()
    ei, ev, _ = batch(lambda eng: None)
    gi, gv, got = batch(lambda eng: _match(torch, eng, c.table, c.preds, m.rows, wait=False))
    assert np.array_equal(gi, ei) and np.array_equal(gv, ev)
    _same(got, c.exp, "cross_talk", m.rows)


def test_per_partition_engine_is_served(pkg, cases):
    """An approximate per-partition engine (partitions > 1) gives the exact engine's masks; with dev_mask it is unsupported, as
    filtered queries are."""
    import torch
    c = cases(1)
    m = c.m
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, partitions=4, k_per_partition=8)
    try:
        _same(_match(torch, eng, c.table, c.preds, m.rows), c.exp, "partitions", m.rows)
        dmask = _dev(torch, pkg.row_mask(m.rows))
        with pytest.raises(pkg.TkspmvError) as e:
            _match(torch, eng, c.table, c.preds, m.rows, dmask=dmask)
        assert e.value.status == pkg._lib.ERR_UNSUPPORTED
    finally:
        eng.close()


def test_errors(pkg, cases):
    import torch
    c = cases(0)
    m, eng = c.m, c.eng
    words = (m.rows + 31) // 32
    dt = _dev(torch, np.tile(c.table, 2))
    dp = _dev(torch, _pred_array(c.preds[:2]).ravel())
    do = _dev(torch, np.zeros(2 * words + 4, dtype=np.uint32))
    torch.cuda.synchronize()
    T, P, O = dt.data_ptr(), dp.data_ptr(), do.data_ptr()

    def status_of(fn):
        with pytest.raises(pkg.TkspmvError) as e:
            fn()
        return e.value.status
    INV = pkg._lib.ERR_INVALID
    assert status_of(lambda: eng.enqueue_match(0, P, 1, O)) == INV                                   # no table
    assert status_of(lambda: eng.enqueue_match(T, 0, 1, O)) == INV                                   # no predicates
    assert status_of(lambda: eng.enqueue_match(T, P, 1, 0)) == INV                                   # no output
    assert status_of(lambda: eng.enqueue_match(T, P, 0, O)) == INV                                   # count < 1
    assert status_of(lambda: eng.enqueue_match(T, P, 1, O, clause_stride=-1)) == INV                 # negative strides
    assert status_of(lambda: eng.enqueue_match(T, P, 1, O, mask_stride=-1)) == INV
    assert status_of(lambda: eng.enqueue_match(T, P, 1, O, out_stride=-1)) == INV
    assert status_of(lambda: eng.enqueue_match(T, P, 2, O, out_stride=words, clause_stride=m.cols - 1)) == INV   # neither 0 nor >= cols
    assert status_of(lambda: eng.enqueue_match(T, P, 2, O, out_stride=words - 1)) == INV             # below words
    assert status_of(lambda: eng.enqueue_match(T, P, 2, O, out_stride=0)) == INV                     # 0 with count != 1
    f16 = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, precision=pkg.F16)
    try:
        assert status_of(lambda: f16.enqueue_match(T, P, 1, O)) == pkg._lib.ERR_UNSUPPORTED
        assert status_of(lambda: f16.match(c.table, c.preds[0])) == pkg._lib.ERR_UNSUPPORTED
    finally:
        f16.close()
    # and the valid forms of the same calls go through
    eng.enqueue_match(T, P, 2, O, out_stride=words + 2, clause_stride=m.cols)
    eng.enqueue_match(T, P, 1, O, out_stride=0)
    eng.synchronize()
