"""Scores of given rows (tkspmv_enqueue_score_rows / tkspmv_score_rows, SpMV.score_rows / rerank) on the MI355X.

Everything is compared bit for bit: the expected score of (query, row) is the order-matched oracle's y[row] over the engine's own
layout (oracle.packed_scores of the WHOLE stream), +0.0 for a row without entries, -inf (0xFF800000) for an id outside the
engine's rows. The queries of the bit comparison are signed (standard normal), so the order of the sums shows in the bits; a gold
leg with the project's non-negative sample vector compares with the fp64 scores. On top: identities with the other paths of one
engine (tkspmv_scores, the top-k lists of enqueue_batch, row_vectors as queries).
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

import support
from support import Layout, bits, coo

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's north-star tolerance (test_gpu_range.py)
FILL, GUARD = -7.0, 1024
OUTSIDE = 0xFFFFFFFF
NEG_INF_BITS = 0xFF800000
GAP = 0xABCD1234  # what lies between the lists of a strided id buffer


LONG = {100: 256, 101: 512, 102: 1500}  # rows rewritten with exactly this many entries
TRIPLE = 200                            # a row with one column three times (and another twice)


def _matrix(pkg, rows, cols, seed, dist="gamma"):
    """A generated matrix with the special rows the tests ask for: long rows (LONG), empty rows in front (1, 2), in the middle
    (rows // 2) and at the end (the last two: they have no packets at all), a row with a column three times (TRIPLE)."""
    g = pkg.generate_matrix(rows, cols, 20, dist, seed)
    rng = np.random.default_rng(seed)
    empty = {1, 2, rows // 2, rows - 2, rows - 1}
    drop = np.isin(g.row, list(empty | set(LONG) | {TRIPLE}))
    row, col, val = [g.row[~drop]], [g.col[~drop]], [g.val[~drop]]
    for r, n in LONG.items():
        row.append(np.full(n, r, np.uint32))
        col.append(rng.integers(0, cols, n).astype(np.uint32))  # (with replacement: 1500 entries repeat many columns)
        val.append((rng.random(n) * 0.1).astype(np.float32))
    c3, c2 = 7 % cols, 11 % cols
    tc = np.array([c3, 5, c2, c3, 9, c2, 3, c3, 13], dtype=np.uint32) % cols
    row.append(np.full(tc.size, TRIPLE, np.uint32))
    col.append(tc)
    val.append(np.array([0.1, 0.3, 1e-8, 0.7, 0.2, 0.5, 0.05, 1e-9, 0.6], dtype=np.float32))  # (sums whose order shows in the bits)
    row, col, val = np.concatenate(row), np.concatenate(col), np.concatenate(val)
    order = np.argsort(row, kind="stable")
    return coo(pkg, rows, cols, row[order], col[order], val[order]), sorted(empty)


def _rows_with_repeats(m, want=5):
    """Short rows (outside LONG / TRIPLE) in which a column occurs more than once."""
    key = m.row.astype(np.uint64) * np.uint64(1 << 20) + m.col.astype(np.uint64)
    u, cnt = np.unique(key, return_counts=True)
    rr = np.unique((u[cnt > 1] >> np.uint64(20)).astype(np.int64))
    return [int(r) for r in rr if r not in LONG and r != TRIPLE][:want]


def _special_ids(m, empties, layout, first_row):
    rep = _rows_with_repeats(m)
    assert len(rep) >= 3, "the input has no rows with a repeated column: the case shows nothing"
    cols_of_triple = m.col[m.row == TRIPLE]
    assert np.max(np.unique(cols_of_triple, return_counts=True)[1]) == 3
    for r, n in LONG.items():
        assert int(np.count_nonzero(m.row == r)) == n
    for r in empties:
        assert not np.any(m.row == r)
    local = [0, m.rows - 1] + layout.partition_rows() + list(LONG) + list(empties) + rep + [TRIPLE]
    ids = [first_row + r for r in local]
    outside = [first_row + m.rows, first_row + m.rows + 12345, OUTSIDE] + ([first_row - 1, 0] if first_row else [])
    return ids + outside + [ids[3], ids[3], first_row + 102, ids[3]]  # (the same id several times in one call)


class _Expect:
    """Expected scores of one engine: the oracle's full-stream scores of a query, computed once per query vector."""
    def __init__(self, oracle, layout, rows, first_row):
        self.oracle, self.layout, self.rows, self.first_row = oracle, layout, rows, first_row
        self.cache = {}

    def full(self, x):
        key = x.tobytes()
        if key not in self.cache:
            self.cache[key] = self.layout.scores(self.oracle, x)
        return self.cache[key]

    def bits(self, xs, ids):
        """uint32 [count, n_rows]; ids: [n_rows] (one list) or [count, n_rows]."""
        ids = np.asarray(ids, dtype=np.int64)
        out = np.zeros((xs.shape[0], ids.shape[-1]), dtype=np.uint32)
        for q in range(xs.shape[0]):
            yp, present = self.full(xs[q])
            lst = ids if ids.ndim == 1 else ids[q]
            r = lst - self.first_row
            inside = (r >= 0) & (r < self.rows)
            rc = np.where(inside, r, 0)
            out[q] = np.where(inside, np.where(present[rc], bits(yp)[rc], 0), NEG_INF_BITS)
        return out


def _run(torch, eng, xs, ids, stride=0, stream=None):
    """One enqueue_score_rows call into a pattern-filled buffer with a guard zone behind it. ids: [n_rows] with stride 0, or
    [count, n_rows] laid out with `stride` >= n_rows words per list (the gap holds GAP). Returns the host copy of the scores."""
    ids = np.asarray(ids, dtype=np.uint32)
    count, n_rows = xs.shape[0], ids.shape[-1]
    if stride == 0:
        assert ids.ndim == 1
        buf = ids.copy()
    else:
        buf = np.full((count, stride), GAP, dtype=np.uint32)
        buf[:, :n_rows] = ids
    d_xs = torch.from_numpy(np.ascontiguousarray(xs, dtype=np.float32)).cuda()
    d_ids = torch.from_numpy(buf.view(np.int32)).cuda()
    d_out = torch.full((count * n_rows + GUARD,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if stream is None:
        eng.enqueue_score_rows(d_xs.data_ptr(), count, d_ids.data_ptr(), n_rows, d_out.data_ptr(), rows_stride=stride)
        eng.synchronize()
    else:
        eng.enqueue_score_rows(d_xs.data_ptr(), count, d_ids.data_ptr(), n_rows, d_out.data_ptr(), rows_stride=stride, stream=stream.cuda_stream)
        stream.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), buf), "the id buffer changed"
    out = d_out.cpu().numpy()
    assert np.all(bits(out[count * n_rows:]) == bits(np.float32(FILL))), "written beyond count x n_rows"
    return out[:count * n_rows].reshape(count, n_rows)


def _check(torch, eng, expect, xs, ids, label, stride=0, stream=None):
    got = bits(_run(torch, eng, xs, ids, stride, stream))
    want = expect.bits(xs, ids)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{label}: {bad.shape[0]} scores differ, first (query, position) {bad[:6].tolist()}: got {got[tuple(bad[0])]:#x}, expected {want[tuple(bad[0])]:#x}"
    return got


def _signed_queries(n, cols, seed):
    return np.random.default_rng(seed).standard_normal((n, cols)).astype(np.float32)


CONFIGS = [
    ("c12_1024", dict(rows=30000, cols=1024, seed=3), dict()),
    ("f32_4096", dict(rows=20000, cols=4096, seed=4), dict()),
    ("f32_16384", dict(rows=6000, cols=16384, seed=5), dict()),
    ("c8_1024", dict(rows=30000, cols=1024, seed=6), dict(nnz_per_lane=8)),
    ("c12_300", dict(rows=20000, cols=300, seed=7, dist="uniform"), dict()),
    ("first_row", dict(rows=30000, cols=512, seed=8), dict(first_row=1_000_000)),
    ("from_packed", dict(rows=30000, cols=1024, seed=9), dict()),
]


@pytest.mark.parametrize("name,mk,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_score_rows(pkg, oracle, tmp_path, name, mk, kw):
    import torch
    m, empties = _matrix(pkg, **mk)
    first_row = kw.get("first_row", 0)
    packed = None
    if name == "from_packed":
        hint = pkg.Packed.wave_partitions(device=0, m=m)
        packed = pkg.Packed(m, k=16, n_wave_partitions=hint)
        packed.save(tmp_path / "m.tkspmv")
        eng = pkg.SpMV.from_packed(pkg.Packed.load(tmp_path / "m.tkspmv"), k=16, device=0)
    else:
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=16, device=0, **kw)
    assert eng.info()["packet_entries"] == (512 if name == "c8_1024" else 256)
    layout = Layout(pkg, eng, m, packed)
    expect = _Expect(oracle, layout, m.rows, first_row)
    special = _special_ids(m, empties, layout, first_row)
    assert len(special) >= 33
    rng = np.random.default_rng(1)
    many = np.concatenate([np.array(special, dtype=np.uint32), (first_row + rng.integers(0, m.rows, 5000 - len(special))).astype(np.uint32)])
    rng.shuffle(many)
    xs = _signed_queries(33, m.cols, 70)
    side = torch.cuda.Stream()
    # (a) one query, one row: the 1500-entry row
    got = _check(torch, eng, expect, xs[:1], [first_row + 102], f"{name} (a)")
    assert got[0, 0] not in (0, NEG_INF_BITS)
    # (b) three queries, one list of 33
    got = _check(torch, eng, expect, xs[:3], special[:33], f"{name} (b)")
    _check(torch, eng, expect, xs[:3], special[-33:], f"{name} (b, the end of the special ids)")
    # (what the lists are made for does occur: ids outside, rows without entries, rows with entries)
    tail = expect.bits(xs[:1], special)[0]
    assert np.count_nonzero(tail == NEG_INF_BITS) >= 3 and np.count_nonzero(tail == 0) >= 5 and np.count_nonzero((tail != 0) & (tail != NEG_INF_BITS)) >= 20
    # (c) a list per query: 33 x 33, dense and with a gap between the lists
    per_query = np.stack([np.roll(np.array((special * 2)[:66], dtype=np.uint32), q)[:33] for q in range(33)])
    per_query[5] = many[:33]
    _check(torch, eng, expect, xs, per_query, f"{name} (c) stride 33", stride=33)
    _check(torch, eng, expect, xs, per_query, f"{name} (c) stride 40", stride=40, stream=side)
    # (d) two queries, one list of 5000, on a caller's stream
    _check(torch, eng, expect, xs[:2], many, f"{name} (d)", stream=side)
    # the gold leg: the project's non-negative sample vector against the fp64 scores
    xg = pkg.create_sample_vector(m.cols, True, False, True, 11)
    inside = many[(many.astype(np.int64) >= first_row) & (many.astype(np.int64) < first_row + m.rows)]
    got = _run(torch, eng, xg[None, :], inside)[0]
    y64, _ = oracle.scores_f64(m.row, m.col, m.val, xg, m.rows)
    assert np.allclose(got.astype(np.float64), y64[inside.astype(np.int64) - first_row], rtol=RTOL, atol=0), f"{name}: scores differ from fp64"
    assert np.array_equal(bits(got), expect.bits(xg[None, :], inside)[0]), f"{name}: gold-leg scores differ from the order-matched oracle"
    # the host-array call: one list, a list per query, the installed vector
    assert np.array_equal(bits(eng.score_rows(special, xs[:3])), expect.bits(xs[:3], special)), name
    assert np.array_equal(bits(eng.score_rows(per_query[:4], xs[:4])), expect.bits(xs[:4], per_query[:4])), name
    eng.reset(xs[7])
    assert np.array_equal(bits(eng.score_rows(many)), expect.bits(xs[7:8], many)), name
    eng.close()


def test_cross_path_identities(pkg):
    """One engine: score_rows against tkspmv_scores, against the lists of enqueue_batch, and with row vectors as the queries."""
    import torch
    m, _ = _matrix(pkg, 30000, 1024, 13)
    k, first_row = 50, 7000
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, first_row=first_row)
    xs = _signed_queries(3, m.cols, 71)
    all_ids = (first_row + np.arange(m.rows)).astype(np.uint32)
    # every row, against the full score vector of the same query
    for q in range(2):
        eng.reset(xs[q])
        y = eng.scores()
        assert np.array_equal(bits(eng.score_rows(all_ids)[0]), bits(y)), "score_rows of all rows differs from scores()"
        assert np.array_equal(bits(eng.score_rows(all_ids[::-1].copy(), xs[q])[0]), bits(y[::-1]))
    # the top-k lists fed back (non-negative queries: the lists are full of rows with positive scores)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 80 + i) for i in range(4)])
    val, idx = support.batch(torch, eng, xq, k)
    assert np.all(val > 0)
    assert np.array_equal(bits(eng.score_rows(idx, xq)), bits(val)), "the scores of the rows enqueue_batch returned differ from its scores"
    # rows as queries: score_rows(ids, row_vectors(ids)) against scores() with each row vector installed
    ids = (first_row + np.array([100, 101, 102, TRIPLE, 0, 2, 29999, 4711])).astype(np.uint32)
    rv, _ = eng.row_vectors(ids)
    got = eng.score_rows(ids, rv)
    for i in range(ids.size):
        eng.reset(rv[i])
        assert np.array_equal(bits(got[i]), bits(eng.scores()[ids.astype(np.int64) - first_row])), f"row vector {int(ids[i])} as the query"
    eng.close()


def test_approximate_partition_engines_are_served(pkg, oracle):
    m, _ = _matrix(pkg, 20000, 1024, 12)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    ids = np.array([0, 100, 101, 102, TRIPLE, 1, 19999, 20000], dtype=np.uint32)
    xs = _signed_queries(2, m.cols, 72)
    expect = _Expect(oracle, Layout(pkg, eng, m), m.rows, 0)
    assert np.array_equal(bits(eng.score_rows(ids, xs)), expect.bits(xs, ids))
    eng.close()


def test_no_cross_talk(pkg):
    """enqueue_score_rows unwaited right behind a batch launch, a batch launch right behind it, one stream."""
    import torch
    m, _ = _matrix(pkg, 60000, 1024, 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    rng = np.random.default_rng(2)
    ids = np.concatenate([[100, 101, 102, TRIPLE, 0, m.rows - 3, m.rows + 5], rng.integers(0, m.rows, 505)]).astype(np.uint32)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    # the solo runs
    want_q = support.batch(torch, eng, xq, k)
    want_s = eng.score_rows(ids, xq)
    n = ids.size
    d_q = torch.from_numpy(xq).cuda()
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    d_sc = torch.full((8, n), FILL, dtype=torch.float32, device="cuda")
    d_idx0, d_val0 = torch.zeros((8, k), dtype=torch.int32, device="cuda"), torch.zeros((8, k), dtype=torch.float32, device="cuda")
    d_idx1, d_val1 = torch.zeros((8, k), dtype=torch.int32, device="cuda"), torch.zeros((8, k), dtype=torch.float32, device="cuda")
    for stream in (None, torch.cuda.Stream()):
        d_sc.fill_(FILL)
        d_idx0.zero_(), d_val0.zero_(), d_idx1.zero_(), d_val1.zero_()
        torch.cuda.synchronize()
        before = eng.debug_counters()["batch_launches"]
        s = 0 if stream is None else stream.cuda_stream
        eng.enqueue_batch(d_q.data_ptr(), 8, d_idx0.data_ptr(), d_val0.data_ptr(), stream=s)
        eng.enqueue_score_rows(d_q.data_ptr(), 8, d_ids.data_ptr(), n, d_sc.data_ptr(), stream=s)
        eng.enqueue_batch(d_q.data_ptr(), 8, d_idx1.data_ptr(), d_val1.data_ptr(), stream=s)
        if stream is None:
            eng.synchronize()
        else:
            stream.synchronize()
        torch.cuda.synchronize()
        label = "engine's stream" if stream is None else "caller's stream"
        launches = eng.debug_counters()["batch_launches"] - before
        solo = eng.debug_counters()["batch_launches"]
        support.batch(torch, eng, xq, k)
        per_call = eng.debug_counters()["batch_launches"] - solo
        assert launches == 2 * per_call, f"{label}: batch_launches advanced by {launches} for two batch calls of {per_call} each"
        assert np.array_equal(bits(d_sc.cpu().numpy()), bits(want_s)), label
        for d_idx, d_val in ((d_idx0, d_val0), (d_idx1, d_val1)):
            assert np.array_equal(d_idx.cpu().numpy().view(np.uint32), want_q[1]) and np.array_equal(bits(d_val.cpu().numpy()), bits(want_q[0])), label
    eng.close()


def test_score_rows_and_rerank(pkg, oracle):
    m, empties = _matrix(pkg, 20000, 1024, 14)
    first_row = 300
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=10, device=0, first_row=first_row)
    expect = _Expect(oracle, Layout(pkg, eng, m), m.rows, first_row)
    x = _signed_queries(1, m.cols, 73)[0]
    rng = np.random.default_rng(3)
    cand = np.concatenate([first_row + rng.integers(0, m.rows, 300), [first_row + r for r in empties], [first_row - 1, 0, first_row + m.rows, OUTSIDE],
                           [first_row + 102, first_row + 102]]).astype(np.uint32)
    # shapes of score_rows
    assert eng.score_rows(cand, x).shape == (1, cand.size) and eng.score_rows(cand[None, :], x[None, :]).shape == (1, cand.size)
    assert eng.score_rows([], x).shape == (1, 0)
    with pytest.raises(ValueError):
        eng.score_rows(np.zeros((2, 3), np.uint32), x)
    with pytest.raises(ValueError):
        eng.score_rows(cand, x[:-1])
    # rerank: ids outside dropped, score descending then row descending, cut to k
    want_bits = expect.bits(x[None, :], cand)[0]
    keep = want_bits != NEG_INF_BITS
    assert np.count_nonzero(~keep) == 4
    w_ids, w_val = cand[keep], want_bits[keep].view(np.float32)
    order = sorted(range(w_ids.size), key=lambda i: (-float(w_val[i]), -int(w_ids[i])))
    val, idx = eng.rerank(cand, x)
    assert np.array_equal(idx, w_ids[order]) and np.array_equal(bits(val), bits(w_val[order]))
    assert np.all(np.diff(val) <= 0) and np.count_nonzero(val == 0) >= len(empties)
    ties = np.flatnonzero(np.diff(val) == 0)
    assert ties.size >= len(empties) and np.all(idx[ties] >= idx[ties + 1]), "equal scores are ordered by row, descending"
    val5, idx5 = eng.rerank(cand, x, k=5)
    assert np.array_equal(idx5, idx[:5]) and np.array_equal(bits(val5), bits(val[:5]))
    eng.reset(x)
    val_i, idx_i = eng.rerank(cand)  # the installed vector
    assert np.array_equal(idx_i, idx) and np.array_equal(bits(val_i), bits(val))
    v0, i0 = eng.rerank([OUTSIDE, 0], x)
    assert v0.shape == (0,) and i0.shape == (0,)
    eng.close()


def test_errors(pkg):
    import torch
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    d_ids = torch.zeros(64, dtype=torch.int32, device="cuda")
    d_xs = torch.ones((2 * 512,), dtype=torch.float32, device="cuda")
    d_out = torch.full((128,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    INVALID, STATE, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_STATE, pkg._lib.ERR_UNSUPPORTED

    def status_of(fn):
        try:
            fn()
        except pkg.TkspmvError as e:
            return e.status
        return 0

    X, I, O = d_xs.data_ptr(), d_ids.data_ptr(), d_out.data_ptr()
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=prec)
        assert status_of(lambda: eng.enqueue_score_rows(X, 2, I, 4, O)) == UNSUPPORTED, prec
        assert status_of(lambda: eng.score_rows([0, 1], np.ones(512, np.float32))) == UNSUPPORTED, prec
        assert status_of(lambda: eng.rerank([0, 1], np.ones(512, np.float32))) == UNSUPPORTED, prec
        eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    assert status_of(lambda: eng.enqueue_score_rows(X, 2, 0, 4, O)) == INVALID            # no rows
    assert status_of(lambda: eng.enqueue_score_rows(X, 2, I, 4, 0)) == INVALID            # no scores
    assert status_of(lambda: eng.enqueue_score_rows(X, 0, I, 4, O)) == INVALID            # count < 1
    assert status_of(lambda: eng.enqueue_score_rows(X, -1, I, 4, O)) == INVALID
    assert status_of(lambda: eng.enqueue_score_rows(X, 2, I, 0, O)) == INVALID            # n_rows < 1
    assert status_of(lambda: eng.enqueue_score_rows(X, 2, I, -4, O)) == INVALID
    assert status_of(lambda: eng.enqueue_score_rows(X, 2, I, 4, O, rows_stride=-1)) == INVALID
    assert status_of(lambda: eng.enqueue_score_rows(X, 2, I, 4, O, rows_stride=3)) == INVALID  # non-zero and below n_rows
    assert status_of(lambda: eng.enqueue_score_rows(0, 2, I, 4, O)) == INVALID            # the installed vector is one query
    assert status_of(lambda: eng.enqueue_score_rows(0, 1, I, 4, O)) == STATE              # ... and none is installed
    lib = pkg._lib.lib()
    assert lib.tkspmv_score_rows(eng._h, None, 1, None, 4, 0, None) == INVALID
    h_ids, h_out = np.zeros(4, np.uint32), np.full(4, FILL, np.float32)
    assert lib.tkspmv_score_rows(eng._h, None, 1, h_ids.ctypes.data_as(C.POINTER(C.c_uint32)), 4, 0, h_out.ctypes.data_as(C.POINTER(C.c_float))) == STATE
    assert np.all(h_out == FILL)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(bits(d_out.cpu().numpy()) == bits(np.float32(FILL))), "a rejected call wrote its output"
    # accepted: stride equal to n_rows, and the installed vector once there is one
    eng.reset(np.ones(512, np.float32))
    eng.enqueue_score_rows(0, 1, I, 4, O)
    eng.enqueue_score_rows(X, 2, I, 4, O + 64 * 4, rows_stride=4)
    eng.synchronize()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    y0 = eng.scores()[0]
    assert np.all(bits(out[:4]) == bits(y0)) and np.all(bits(out[64:72]) == bits(y0)) and np.all(out[4:64] == FILL) and np.all(out[72:] == FILL)
    eng.close()
