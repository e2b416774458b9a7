"""Search-after paging (tkspmv_enqueue_after / tkspmv_run_after) on the MI355X.

Every result is compared EXACTLY -- row ids, score bits, n, total, the next cursor -- with page_after (host.py), the numpy
restatement of the contract whose ordering tests/test_after_host.py pins to the oracle's selection and to a plain loop. The scores
it pages over are the order-matched oracle's over the engine's own layout for fp32 engines, the engine's own full score vector
(eng.scores()) for the other value types, and plain integer sums for the matrices of ones (exact in any order). The conftest
syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves.

One row of the error table cannot be reached: every engine that can be created holds the packet stream."""
import ctypes as C

import numpy as np
import pytest

import support
from support import GUARD, EngineSetup, PageOut, bits_of, status_of

pytestmark = pytest.mark.gpu

START, AFTER, END = 0, 1, 2


def _same(got, want, what=""):
    idx, val, n, total, nxt = got
    ei, ev, en, et, ec = want
    assert (n, total) == (en, et), (what, n, total, en, et)
    assert np.array_equal(idx, ei), (what, "row ids differ from page_after")
    assert np.array_equal(val.view(np.uint32), ev.view(np.uint32)), (what, "scores are not bit-identical")
    assert np.all(idx[en:] == 0) and np.all(val[en:].view(np.uint32) == 0), (what, "pads")
    assert nxt == ec, (what, nxt, ec)


def _query(eng, torch, dxs, count, cursors=None, stream=0, **kw):
    """enqueue_after into fresh guarded buffers; waits; [(idx, val, n, total, next)] per query."""
    out = PageOut(torch, count, eng.k)
    dcur = support.cursors(torch, cursors) if cursors is not None else None
    torch.cuda.synchronize()
    eng.enqueue_after(dxs.data_ptr() if dxs is not None else 0, count, dev_cursors=dcur.data_ptr() if dcur is not None else 0,
                      stream=stream.cuda_stream if stream else 0, **out.ptrs(), **kw)
    if stream:
        stream.synchronize()
    else:
        eng.synchronize()
    return out.read()


CONFIGS = {
    "default12bit": dict(shape=(20011, 1024, 20), k=100, kw={}),
    "cols4096": dict(shape=(5000, 3000, 30), k=50, kw={}),
    "radix": dict(shape=(1000, 512, 20), k=100, kw={}),
    "c8": dict(shape=(20011, 1024, 20), k=100, kw={"nnz_per_lane": 8}),
    "first_row": dict(shape=(20011, 1024, 20), k=100, kw={"first_row": 5000}),
    "min_score": dict(shape=(20011, 1024, 20), k=100, kw={}, min_rank=30),
    "f16": dict(shape=(20011, 1024, 20), k=100, kw={"precision": "F16"}),
    "q17f32": dict(shape=(20011, 1024, 20), k=100, kw={"precision": "Q1_7_F32"}),
    "fixed20": dict(shape=(20011, 1024, 20), k=100, kw={"precision": "FIXED", "fixed_width": 20}),
    "walk": dict(shape=(2003, 512, 20), k=16, kw={}),
}


def _drop_rows(m, every, which):
    """The matrix without the entries of the rows r % every == which: rows without entries in the middle of the matrix."""
    keep = m.row % every != which
    m.row, m.col, m.val = m.row[keep].copy(), m.col[keep].copy(), m.val[keep].copy()
    return m


class _Setup(EngineSetup):
    """The engine and scores of one of CONFIGS, over a matrix with empty rows in its middle; the expectation pages over the scores."""
    def matrix(self, m):
        return _drop_rows(m, 7, 3)

    def expect(self, pkg, cursor=None, allow=None, y=None, present=None, k=None):
        y = self.y if y is None else y
        present = self.present if present is None else present
        return pkg.page_after(y, present, self.k if k is None else k, cursor, self.min_score, self.first_row, allow)


@pytest.fixture(scope="module", params=[c for c in CONFIGS if c != "walk"])
def setup(request, pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, CONFIGS[request.param])
    yield s
    s.eng.close()


def test_start_is_the_engines_own_topk(pkg, setup):
    import torch
    s, eng = setup, setup.eng
    want = s.expect(pkg)
    got, = _query(eng, torch, s.dx, 1)
    _same(got, want, "dev_cursors = NULL")
    got2, = _query(eng, torch, s.dx, 1, [(12345, 0x3F800000, START)])  # START ignores row and score
    _same(got2, want, "START cursor")
    eng()  # the engine's own top-k
    tv, ti = eng.read_result()
    assert np.array_equal(ti, got[0]) and np.array_equal(tv.view(np.uint32), got[1].view(np.uint32))
    if s.fp32:
        fv, fi = eng.run_filtered(allow=np.ones(s.m.rows, dtype=bool))
        assert np.array_equal(fi, got[0]) and np.array_equal(fv.view(np.uint32), got[1].view(np.uint32))
        eng.set_filter(None)
    if s.min_score != 0.0:
        assert got[2] == got[3] == 30 and got[4] == (0, 0, END)  # fewer eligible rows than a page: pads, and no page follows


def test_mid_order_cursors(pkg, setup):
    import torch
    s, eng, rows = setup, setup.eng, setup.m.rows
    rng = np.random.default_rng(3)
    ranking = s.expect(pkg, k=rows)
    eligible = ranking[2]
    allow = rng.random(rows) < 0.5
    empty = int(np.flatnonzero(~s.present)[5])
    masked = int(np.flatnonzero(s.present & ~allow)[5])
    mid = ranking[1][min(eligible, 2000) // 2]  # a score of the ranking's middle
    cursors = []
    for r in sorted({0, 1, eligible // 3, eligible // 2, eligible - 2, eligible - 1} & set(range(eligible))):
        cursors.append((int(ranking[0][r]), bits_of(ranking[1][r]), AFTER))               # an entry of the ranking itself
    cursors += [(empty + s.first_row, bits_of(mid), AFTER),                                # a row without entries
                (masked + s.first_row, bits_of(s.y[masked]), AFTER),                       # a masked row (for the masked queries below)
                (s.first_row + rows + 1000, bits_of(mid), AFTER), (0xFFFFFFFF, bits_of(mid), AFTER), (0, bits_of(mid), AFTER),  # rows in no shard
                (17, bits_of(np.nextafter(np.float32(mid), np.float32(np.inf))), AFTER),   # a score (most likely) no row has
                (17, bits_of(1e30), AFTER), (17, bits_of(-1.0), AFTER),                      # above every score, below every eligible one
                (17, bits_of(mid), END), (17, bits_of(mid), 0xFFFFFFFF)]                     # END and a state that acts as END
    xs = torch.from_numpy(np.tile(s.x, (len(cursors), 1))).cuda()
    got = _query(eng, torch, xs, len(cursors), cursors)
    for c, g in zip(cursors, got):
        _same(g, s.expect(pkg, c), c)
    assert got[-1][2:] == (0, 0, (0, 0, END)) and got[-2][2:] == (0, 0, (0, 0, END))  # END: all pads, n = 0, total = 0
    assert got[-4][3] == eligible and got[-3][3] == 0
    if s.fp32:  # the same cursors under a mask
        dmask = torch.from_numpy(pkg.row_mask(rows, allow).view(np.int32)).cuda()
        got = _query(eng, torch, xs, len(cursors), cursors, dev_mask=dmask.data_ptr())
        for c, g in zip(cursors, got):
            _same(g, s.expect(pkg, c, allow), ("masked", c))


def _walk(pkg, torch, eng, dx, want_ranking, eligible):
    """ceil(eligible / k) calls with ONE cursor buffer advanced in place, all enqueued before the first wait."""
    k = eng.k
    pages = -(-eligible // k)
    out = PageOut(torch, pages, k)
    cur = support.cursors(torch, [None])
    torch.cuda.synchronize()
    for p in range(pages):
        ptrs = out.ptrs(p)
        ptrs["dev_next"] = cur.data_ptr()
        eng.enqueue_after(dx.data_ptr(), 1, dev_cursors=cur.data_ptr(), **ptrs)
    eng.synchronize()
    out.dev["dev_next"][GUARD:GUARD + 4 * pages] = 0  # (next went to the cursor buffer instead: read() checks the reserved words)
    got = out.read()
    left = eligible
    for p, (idx, val, n, total, _) in enumerate(got):
        assert (n, total) == (min(k, left), left), (p, n, total, left)
        lo = eligible - left
        assert np.array_equal(idx[:n], want_ranking[0][lo:lo + n]), (p, "row ids")
        assert np.array_equal(val[:n].view(np.uint32), want_ranking[1][lo:lo + n].view(np.uint32)), (p, "score bits")
        assert np.all(idx[n:] == 0) and np.all(val[n:].view(np.uint32) == 0), (p, "pads")
        left -= n
    assert left == 0
    assert cur.cpu().numpy().view(np.uint32).tolist() == [[0, 0, END, 0]], "the walk must end as END within ceil(eligible / k) calls"
    return got


def test_full_walk_with_one_cursor_buffer(pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, CONFIGS["walk"])
    ranking = s.expect(pkg, k=s.m.rows)
    eligible = ranking[2]
    assert eligible % s.k != 0 and eligible > 100 * s.k
    got = _walk(pkg, torch, s.eng, s.dx, ranking, eligible)
    assert 0 < got[-1][2] < s.k, "the last page must be short and padded"
    again = _walk(pkg, torch, s.eng, s.dx, ranking, eligible)  # the same walk again: the words were left as they were found
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) for a, b in zip(got, again))
    s.eng.close()


class _Ties:
    """A matrix of ones and a sparse 0/1 query: small integer scores, exact in any order, two tie classes of more than 2048 rows
    (the selection's general path at every cut inside them)."""
    def __init__(self, pkg):
        self.rows, self.cols = 8009, 512
        self.m = _drop_rows(pkg.generate_matrix(self.rows, self.cols, 20, "gamma", 31), 11, 4)
        self.m.val = np.ones_like(self.m.val)
        self.x = (np.random.default_rng(2).random(self.cols) < 0.04).astype(np.float32)
        self.y = np.zeros(self.rows, dtype=np.float32)
        np.add.at(self.y, self.m.row, self.x[self.m.col])  # (sums of at most a few dozen ones: exact)
        self.present = support.present(self.m)
        _, counts = np.unique(self.y[self.present], return_counts=True)
        assert np.sort(counts)[-2] > 2048, "two tie classes must be larger than the selection's LDS list"


@pytest.fixture(scope="module")
def ties(pkg):
    return _Ties(pkg)


def test_full_walk_across_ties(pkg, ties):
    import torch
    t = ties
    eng = pkg.SpMV(t.m.row, t.m.col, t.m.val, t.rows, t.cols, k=16, device=0)
    ranking = pkg.page_after(t.y, t.present, t.rows)
    _walk(pkg, torch, eng, torch.from_numpy(t.x).cuda(), ranking, ranking[2])
    eng.close()


def test_row_sharded_pages_merge_to_the_single_engines(pkg, ties):
    import torch
    from importlib import import_module
    dist = import_module(pkg.__name__ + ".distributed")
    t, k, h = ties, 16, 4001
    lo = t.m.row < h
    whole = pkg.SpMV(t.m.row, t.m.col, t.m.val, t.rows, t.cols, k=k, device=0)
    shards = [pkg.SpMV(t.m.row[lo], t.m.col[lo], t.m.val[lo], h, t.cols, k=k, device=0),
              pkg.SpMV(t.m.row[~lo] - h, t.m.col[~lo], t.m.val[~lo], t.rows - h, t.cols, k=k, device=0, first_row=h)]
    dx = torch.from_numpy(t.x).cuda()
    ranking = pkg.page_after(t.y, t.present, t.rows)
    cursor = None
    for page in range(3):
        single, = _query(whole, torch, dx, 1, [cursor])
        parts = [_query(e, torch, dx, 1, [cursor])[0] for e in shards]  # every shard gets the SAME cursor: ids are global
        gathered = np.stack([np.stack([p[0].view(np.int32), p[1].view(np.int32)]) for p in parts])  # [world][2][k]
        torch.cuda.synchronize()
        mi, mv = dist.merge_topk_device(torch.from_numpy(gathered).cuda(), 2, k)
        torch.cuda.synchronize()
        mi, mv = mi.cpu().numpy().view(np.uint32), mv.cpu().numpy()
        assert np.array_equal(mi, single[0]) and np.array_equal(mv.view(np.uint32), single[1].view(np.uint32)), page
        assert np.array_equal(mi, ranking[0][page * k:(page + 1) * k]), page
        assert sum(p[3] for p in parts) == single[3] > k
        cursor = (int(mi[k - 1]), int(mv.view(np.uint32)[k - 1]), AFTER)  # the shards' totals sum to more than k: AFTER(last merged entry)
        assert cursor == single[4]
        assert any(p[4] != cursor for p in parts), "a shard's own next cursor is not the global one"
    for e in shards + [whole]:
        e.close()


@pytest.fixture(scope="module")
def plain(pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, CONFIGS["default12bit"])
    yield s
    s.eng.close()


def test_masks_and_cursors_per_query(pkg, oracle, plain):
    import torch
    s, eng, rows = plain, plain.eng, plain.m.rows
    rng = np.random.default_rng(8)
    for density in (0.5, 0.001):
        allow = rng.random(rows) < density
        dmask = torch.from_numpy(pkg.row_mask(rows, allow).view(np.int32)).cuda()
        top = s.expect(pkg, None, allow)
        cursor = (int(top[0][min(top[2], 7) - 1]), bits_of(top[1][min(top[2], 7) - 1]), AFTER)  # behind the 7th allowed row
        got = _query(eng, torch, torch.from_numpy(np.tile(s.x, (2, 1))).cuda(), 2, [None, cursor], dev_mask=dmask.data_ptr())
        _same(got[0], top, f"mask {density}")
        _same(got[1], s.expect(pkg, cursor, allow), f"mask {density}, cursor")
        assert got[1][3] == got[0][3] - min(top[2], 7)
    # five queries in one call: a vector, a mask (with a stride) and a cursor each
    xs = np.stack([pkg.create_sample_vector(s.m.cols, True, False, True, 70 + i) for i in range(5)]).astype(np.float32)
    allows = [rng.random(rows) < d for d in (0.5, 0.02, 0.9, 0.001, 1.0)]
    words = np.stack([pkg.row_mask(rows, a) for a in allows])
    dmask = torch.from_numpy(words.view(np.int32)).cuda()
    scores = [s.scores(oracle, xs[q]) for q in range(5)]
    cursors = [None]
    for q in range(1, 5):  # behind rank 10 * q of the query's own masked ranking (END where the mask leaves fewer rows)
        r = pkg.page_after(*scores[q], 10 * q, None, 0.0, 0, allows[q])
        cursors.append(r[4] if r[4][2] == AFTER else (0, 0, END))
    dxs = torch.from_numpy(xs).cuda()
    side = torch.cuda.Stream()
    first = _query(eng, torch, dxs, 5, cursors, stream=side, dev_mask=dmask.data_ptr(), mask_stride=words.shape[1])
    second = _query(eng, torch, dxs, 5, cursors, stream=side, dev_mask=dmask.data_ptr(), mask_stride=words.shape[1])
    for q in range(5):
        _same(first[q], s.expect(pkg, cursors[q], allows[q], *scores[q]), f"query {q}")
        _same(second[q], first[q], f"query {q} again")  # the same call again: identical bits
    assert sum(c is not None and c[2] == AFTER for c in cursors) >= 3


def test_no_cross_talk_with_the_batch_path_and_read(pkg, oracle, plain):
    import torch
    s, eng, k = plain, plain.eng, plain.k
    nq = 40
    xs = np.stack([pkg.create_sample_vector(s.m.cols, True, False, True, 200 + i) for i in range(nq)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    b_i = [torch.zeros((nq, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    b_v = [torch.zeros((nq, k), dtype=torch.float32, device="cuda") for _ in range(2)]
    scores = [s.scores(oracle, xs[q]) for q in range(nq)]
    tops = {q: s.expect(pkg, None, None, *scores[q]) for q in (2, 7, 8, 11)}
    cursors = [tops[7][4], tops[8][4]]  # page 2 of queries 7 and 8
    dcur = support.cursors(torch, cursors)
    out = PageOut(torch, 2, k)
    torch.cuda.synchronize()
    # an unwaited batch sequence, the after call right behind it, another batch sequence right behind that: one stream, one wait
    eng.enqueue_batch(dxs.data_ptr(), nq, b_i[0].data_ptr(), b_v[0].data_ptr())
    eng.enqueue_after(dxs.data_ptr() + 4 * 7 * s.m.cols, 2, dev_cursors=dcur.data_ptr(), **out.ptrs())
    eng.enqueue_batch(dxs.data_ptr(), nq, b_i[1].data_ptr(), b_v[1].data_ptr())
    eng.synchronize()
    for q in range(nq):
        ei, ev = oracle.select_topk(scores[q][0], scores[q][1].astype(np.uint8), k)
        for j in range(2):
            assert np.array_equal(b_i[j][q].cpu().numpy().view(np.uint32), ei), (j, q)
            assert np.array_equal(b_v[j][q].cpu().numpy().view(np.uint32), ev.view(np.uint32)), (j, q)
    for j, q in enumerate((7, 8)):
        _same(out.read()[j], s.expect(pkg, cursors[j], None, *scores[q]), f"after query {q}")
    before = eng.debug_counters()
    # engine-owned outputs: tkspmv_read returns the page (the last query wins), pads included
    dcur3 = support.cursors(torch, [None, None, tops[2][4]])
    torch.cuda.synchronize()
    eng.enqueue_after(dxs.data_ptr(), 3, dev_cursors=dcur3.data_ptr())
    eng.synchronize()
    rv, ri = eng.read_result()
    want = s.expect(pkg, tops[2][4], None, *scores[2])
    assert np.array_equal(ri, want[0]) and np.array_equal(rv.view(np.uint32), want[1].view(np.uint32))
    # the host form: the installed vector, a host cursor; tkspmv_read sees its page too
    eng.reset(xs[11])
    got = eng.run_after(tops[11][4])
    want = s.expect(pkg, tops[11][4], None, *scores[11])
    _same(got, want, "run_after")
    rv, ri = eng.read_result()
    assert np.array_equal(ri, want[0]) and np.array_equal(rv.view(np.uint32), want[1].view(np.uint32))
    _same(eng.run_after(), tops[11], "run_after from the top")
    after = eng.debug_counters()
    for key in ("checks_failed", "late_repairs", "single_repairs", "single_checks_failed", "batch_launches", "single_launches"):
        assert after[key] == before[key], (key, before, after)  # the after calls ran no batch or single launch and failed no check
    # ... and the batch path still answers exactly behind them
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), nq, b_i[0].data_ptr(), b_v[0].data_ptr())
    eng.synchronize()
    ei, ev = oracle.select_topk(scores[nq - 1][0], scores[nq - 1][1].astype(np.uint8), k)
    assert np.array_equal(b_i[0][nq - 1].cpu().numpy().view(np.uint32), ei)
    eng.reset(s.x)


def test_run_after_pages_and_ranked_spmv(pkg, ties):
    t = ties
    allow = np.random.default_rng(4).random(t.rows) < 0.6
    eng = pkg.SpMV(t.m.row, t.m.col, t.m.val, t.rows, t.cols, k=1000, device=0, vec=t.x)
    for a in (None, allow):
        ranking = pkg.page_after(t.y, t.present, t.rows, allow=a)
        eligible = ranking[2]
        first = eng.run_after(allow=a)
        _same(first, pkg.page_after(t.y, t.present, 1000, allow=a), "run_after from the top")
        second = eng._run_after(first[4], a is not None)
        _same(second, pkg.page_after(t.y, t.present, 1000, first[4], allow=a), "run_after, page 2")
        pages = list(eng.pages(allow=a))
        assert len(pages) == -(-eligible // 1000) and all(v.size == 1000 for v, _ in pages[:-1]) and 0 < pages[-1][0].size < 1000
        assert np.array_equal(np.concatenate([i for _, i in pages]), ranking[0][:eligible])
        assert np.array_equal(np.concatenate([v for v, _ in pages]).view(np.uint32), ranking[1][:eligible].view(np.uint32))
    eng.set_filter(None)
    assert list(eng.pages(allow=np.zeros(t.rows, dtype=bool))) == []  # no eligible row: no page at all
    eng.close()
    ranking = pkg.page_after(t.y, t.present, t.rows)
    val, idx = pkg.ranked_spmv(t.m, t.x, 2500)  # beyond TKSPMV_MAX_K: three pages of the helper's own engine
    assert idx.size == 2500 and np.array_equal(idx, ranking[0][:2500]) and np.array_equal(val.view(np.uint32), ranking[1][:2500].view(np.uint32))
    val, idx = pkg.ranked_spmv(t.m, t.x, 10 * t.rows, k=777, allow=allow)  # more than there is: every eligible row
    ranking = pkg.page_after(t.y, t.present, t.rows, allow=allow)
    assert idx.size == ranking[2] and np.array_equal(idx, ranking[0][:ranking[2]])


def test_errors(pkg):
    import torch
    L = pkg._lib
    m = pkg.generate_matrix(20011, 1024, 20, "gamma", 4)
    x = pkg.create_sample_vector(1024, True, False, True, 2)
    rows, k = m.rows, 100
    dmask = torch.from_numpy(pkg.row_mask(rows).view(np.int32)).cuda()
    buf = torch.zeros(k, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0)
    assert status_of(pkg, eng.enqueue_after, 0, 1) == L.ERR_STATE    # no query vector installed
    assert status_of(pkg, eng.run_after) == L.ERR_STATE
    assert status_of(pkg, eng.enqueue_after, 0, 2) == L.ERR_INVALID  # NULL dev_xs takes the installed vector: count must be 1
    eng.reset(x)
    assert status_of(pkg, eng.enqueue_after, 0, 2) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_after, 0, 0) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_after, 0, -3) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_after, 0, 1, 0, dmask.data_ptr(), -1) == L.ERR_INVALID  # a negative stride
    for given in ((1, 0), (0, 1)):  # output pointers partly given
        p = [buf.data_ptr() if g else 0 for g in given]
        assert status_of(pkg, eng.enqueue_after, 0, 1, 0, 0, 0, *p) == L.ERR_INVALID
    n = C.c_int32(5)
    assert L.lib().tkspmv_run_after(eng._h, None, 1, None, None, C.byref(n), None, None) == L.ERR_INVALID  # use_filter, none installed
    assert n.value == 5
    idx, val, cnt, total, nxt = eng.run_after()  # ... and the engine still answers
    assert cnt == k and total > k and nxt[2] == AFTER
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0, partitions=4, k_per_partition=8)  # the approximate per-partition path
    eng.reset(x)
    assert status_of(pkg, eng.run_after) == L.ERR_UNSUPPORTED
    assert status_of(pkg, eng.enqueue_after, 0, 1) == L.ERR_UNSUPPORTED
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0, precision=pkg.F16)
    eng.reset(x)
    eng.run_after()  # served without a mask ...
    assert status_of(pkg, eng.enqueue_after, 0, 1, 0, dmask.data_ptr()) == L.ERR_UNSUPPORTED  # ... a mask needs the filter kernels
    with pytest.raises(pkg.TkspmvError) as e:
        eng.enqueue_after(0, 1, 0, dmask.data_ptr())
    assert "filtered queries need fp32 values" in str(e.value)
    eng.close()
