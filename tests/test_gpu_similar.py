"""Queries by stored row (tkspmv_enqueue_row_vectors / tkspmv_row_vectors / tkspmv_run_similar, knn_graph) on the MI355X.

Everything is compared bit for bit. The expected vector of a row comes from the COO alone: a zeroed float32 array and np.add.at
over the row's entries in COO order -- sequential fp32 addition from +0.0, which is the contract for repeated columns. A query
on such a vector goes through unchanged code: `similar` must equal enqueue_batch on host-densified vectors of the same engine,
and the order-matched oracle (oracle.packed_scores of the engine's own layout + select_topk).
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import support
from support import Layout, bits, coo

pytestmark = pytest.mark.gpu

FILL_X, FILL_LEN, GUARD = -7.0, 12345, 1024
OUTSIDE = 0xFFFFFFFF


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


class _Rows:
    """Row slices of a row-sorted COO and the expected dense vectors."""
    def __init__(self, m, first_row=0):
        self.m, self.first_row = m, first_row
        self.starts = np.searchsorted(m.row, np.arange(m.rows + 1), side="left")

    def length(self, g):
        r = int(g) - self.first_row
        return OUTSIDE if not 0 <= r < self.m.rows else int(self.starts[r + 1] - self.starts[r])

    def vectors(self, ids):
        xs = np.zeros((len(ids), self.m.cols), dtype=np.float32)
        ln = np.zeros(len(ids), dtype=np.uint32)
        cache = {}
        for i, g in enumerate(ids):
            g = int(g)
            ln[i] = self.length(g)
            if ln[i] in (0, OUTSIDE):
                continue
            if g not in cache:
                a, b = self.starts[g - self.first_row], self.starts[g - self.first_row + 1]
                v = np.zeros(self.m.cols, dtype=np.float32)
                np.add.at(v, self.m.col[a:b], self.m.val[a:b])
                cache[g] = v
            xs[i] = cache[g]
        return xs, ln

    def rows_with_repeats(self, want=5):
        """Short rows (outside LONG / TRIPLE) in which a column occurs more than once."""
        m = self.m
        key = m.row.astype(np.uint64) * np.uint64(1 << 20) + m.col.astype(np.uint64)
        u, cnt = np.unique(key, return_counts=True)
        rr = np.unique((u[cnt > 1] >> np.uint64(20)).astype(np.int64))
        rr = [int(r) for r in rr if r not in LONG and r != TRIPLE]
        return rr[:want]


def _special_ids(m, empties, rows_helper, layout, first_row):
    rep = rows_helper.rows_with_repeats()
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


def _run_row_vectors(torch, eng, ids, cols, stream=None):
    """One enqueue_row_vectors call into pattern-filled buffers with a guard zone behind them. Returns host copies."""
    n = len(ids)
    d_ids = torch.from_numpy(np.asarray(ids, dtype=np.uint32).view(np.int32)).cuda()
    d_xs = torch.full((n * cols + GUARD,), FILL_X, dtype=torch.float32, device="cuda")
    d_len = torch.full((n + GUARD,), FILL_LEN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if stream is None:
        eng.enqueue_row_vectors(d_ids.data_ptr(), n, d_xs.data_ptr(), d_len.data_ptr())
        eng.synchronize()
    else:
        eng.enqueue_row_vectors(d_ids.data_ptr(), n, d_xs.data_ptr(), d_len.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
    return d_xs.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)


def _check_row_vectors(torch, eng, helper, ids, cols, label, stream=None):
    xs, ln = _run_row_vectors(torch, eng, ids, cols, stream)
    n = len(ids)
    exp_xs, exp_ln = helper.vectors(ids)
    assert np.all(bits(xs[n * cols:]) == bits(np.float32(FILL_X))), f"{label}: written beyond count x cols"
    assert np.all(ln[n:] == FILL_LEN), f"{label}: lengths written beyond count"
    assert np.array_equal(ln[:n], exp_ln), f"{label}: lengths differ at {np.flatnonzero(ln[:n] != exp_ln)[:8]}"
    got = bits(xs[:n * cols]).reshape(n, cols)
    bad = np.flatnonzero(np.any(got != bits(exp_xs), axis=1))
    assert bad.size == 0, f"{label}: vectors differ for ids {[int(ids[i]) for i in bad[:8]]} (positions {bad[:8]})"


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
def test_row_vectors(pkg, tmp_path, name, mk, kw):
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
    info = eng.info()
    assert info["packet_entries"] == (512 if name == "c8_1024" else 256)
    helper, layout = _Rows(m, first_row), Layout(pkg, eng, m, packed)
    special = _special_ids(m, empties, helper, layout, first_row)
    assert len(special) >= 33
    rng = np.random.default_rng(1)
    many = np.concatenate([np.array(special, dtype=np.uint32), (first_row + rng.integers(0, m.rows, 5000 - len(special))).astype(np.uint32)])
    rng.shuffle(many)
    side = torch.cuda.Stream()
    _check_row_vectors(torch, eng, helper, [first_row + 102], m.cols, f"{name} count=1 (1500 entries)")
    _check_row_vectors(torch, eng, helper, [special[-5]], m.cols, f"{name} count=1 (outside)", stream=side)
    _check_row_vectors(torch, eng, helper, special[:33], m.cols, f"{name} count=33")
    _check_row_vectors(torch, eng, helper, special[-33:], m.cols, f"{name} count=33, caller's stream", stream=side)
    _check_row_vectors(torch, eng, helper, many, m.cols, f"{name} count=5000")
    _check_row_vectors(torch, eng, helper, many[::-1].copy(), m.cols, f"{name} count=5000, caller's stream", stream=side)
    # the host-array call
    xs, ln = eng.row_vectors(special)
    exp_xs, exp_ln = helper.vectors(special)
    assert np.array_equal(ln, exp_ln) and np.array_equal(bits(xs), bits(exp_xs)), name
    eng.close()


def test_approximate_partition_engines_are_served(pkg):
    m, _ = _matrix(pkg, 20000, 1024, 12)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=32, partitions=8, k_per_partition=8, device=0)
    ids = [0, 100, 101, 102, TRIPLE, 19999, 20000]
    xs, ln = eng.row_vectors(ids)
    exp_xs, exp_ln = _Rows(m).vectors(ids)
    assert np.array_equal(ln, exp_ln) and np.array_equal(bits(xs), bits(exp_xs))
    eng.close()


def test_no_cross_talk(pkg):
    """enqueue_row_vectors unwaited right behind a batch launch, enqueue_batch on its output right behind it, one stream."""
    import torch
    m, _ = _matrix(pkg, 60000, 1024, 21)
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    rng = np.random.default_rng(2)
    ids = np.concatenate([[100, 101, 102, TRIPLE, 0, m.rows - 3], rng.integers(0, m.rows, 42)]).astype(np.uint32)
    xq = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 60 + i) for i in range(8)])
    # the waited run
    want_q = support.batch(torch, eng, xq, k)
    rv, _ = eng.row_vectors(ids)
    want_r = support.batch(torch, eng, rv, k)
    # the unwaited sequence
    n = ids.size
    d_q = torch.from_numpy(xq).cuda()
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    d_rv = torch.full((n, m.cols), FILL_X, dtype=torch.float32, device="cuda")
    d_idx0, d_val0 = torch.zeros((8, k), dtype=torch.int32, device="cuda"), torch.zeros((8, k), dtype=torch.float32, device="cuda")
    d_idx1, d_val1 = torch.zeros((n, k), dtype=torch.int32, device="cuda"), torch.zeros((n, k), dtype=torch.float32, device="cuda")
    for stream in (None, torch.cuda.Stream()):
        d_rv.fill_(FILL_X)
        d_idx0.zero_(), d_val0.zero_(), d_idx1.zero_(), d_val1.zero_()
        torch.cuda.synchronize()
        s = 0 if stream is None else stream.cuda_stream
        eng.enqueue_batch(d_q.data_ptr(), 8, d_idx0.data_ptr(), d_val0.data_ptr(), stream=s)
        eng.enqueue_row_vectors(d_ids.data_ptr(), n, d_rv.data_ptr(), stream=s)
        eng.enqueue_batch(d_rv.data_ptr(), n, d_idx1.data_ptr(), d_val1.data_ptr(), stream=s)
        if stream is None:
            eng.synchronize()
        else:
            stream.synchronize()
        label = "engine's stream" if stream is None else "caller's stream"
        assert np.array_equal(bits(d_rv.cpu().numpy()), bits(rv)), label
        assert np.array_equal(d_idx0.cpu().numpy().view(np.uint32), want_q[1]) and np.array_equal(bits(d_val0.cpu().numpy()), bits(want_q[0])), label
        assert np.array_equal(d_idx1.cpu().numpy().view(np.uint32), want_r[1]) and np.array_equal(bits(d_val1.cpu().numpy()), bits(want_r[0])), label
    eng.close()


def _oracle_lists(oracle, layout, xs, k, first_row=0):
    """The order-matched oracle's top-k of every vector (one full pass over the matrix each: spread over the CPUs)."""
    idx = np.zeros((xs.shape[0], k), dtype=np.uint32)
    val = np.zeros((xs.shape[0], k), dtype=np.float32)

    def one(i):
        yp, present = layout.scores(oracle, xs[i])
        idx[i], val[i] = oracle.select_topk(yp, present, k, 0.0, first_row)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(one, range(xs.shape[0])))
    return val, idx


def _without_self(val, idx, ids):
    """The plain lists with the query's own row removed, the rest moved up, the pad (0, 0.0) at the end."""
    val, idx = val.copy(), idx.copy()
    k = idx.shape[1]
    for i, g in enumerate(ids):
        hit = np.flatnonzero(idx[i] == g)
        if hit.size:
            j = int(hit[0])
            idx[i, j:k - 1], val[i, j:k - 1] = idx[i, j + 1:].copy(), val[i, j + 1:].copy()
            idx[i, k - 1], val[i, k - 1] = 0, 0.0
    return val, idx


@pytest.mark.parametrize("rows,k,n_ids,first_row", [(200_000, 50, 3000, 0), (1_000_000, 100, 64, 0), (50_000, 20, 700, 5_000_000)],
                         ids=["200k_3000rows", "1M_64rows", "first_row"])
def test_similar(pkg, oracle, rows, k, n_ids, first_row):
    import torch
    m, empties = _matrix(pkg, rows, 1024, 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, first_row=first_row)
    helper, layout = _Rows(m, first_row), Layout(pkg, eng, m)
    rng = np.random.default_rng(5)
    special = [100, 101, 102, TRIPLE, 0, empties[0], rows // 2, rows - 1, rows - 3]
    ids = (first_row + np.concatenate([special, rng.integers(0, rows, n_ids - len(special))])).astype(np.uint32)
    before = eng.debug_counters()
    val, idx = eng.similar(ids)
    after = eng.debug_counters()
    # (checks of the batch kernel's local thresholds may fail on such queries: the repair path is part of the contract, and the
    #  lists are compared only now that the call has returned)
    assert after["checks_failed"] >= before["checks_failed"] and after["batch_launches"] >= before["batch_launches"]
    xs, _ = helper.vectors(ids)
    bval, bidx = support.batch(torch, eng, xs, k)
    assert np.array_equal(idx, bidx) and np.array_equal(bits(val), bits(bval)), "similar differs from enqueue_batch on host-densified vectors"
    oval, oidx = _oracle_lists(oracle, layout, xs, k, first_row)
    assert np.array_equal(idx, oidx) and np.array_equal(bits(val), bits(oval)), "similar differs from the order-matched oracle"
    xval, xidx = eng.similar(ids, exclude_self=True)
    eval_, eidx = _without_self(val, idx, ids)
    assert np.array_equal(xidx, eidx) and np.array_equal(bits(xval), bits(eval_))
    # (the generator's rows have norm 1: a row with entries is its own best match, so the removal above did happen)
    assert np.count_nonzero(np.any(idx == ids[:, None], axis=1)) > n_ids // 2
    eng.close()


def test_exclude_self_keeps_a_list_without_the_row(pkg, oracle):
    """A short, low-norm row in a matrix whose other rows are not normalised is not in its own top-k: its list stays as it is."""
    g = pkg.generate_matrix(20000, 1024, 20, "gamma", 41)
    rng = np.random.default_rng(41)
    scale = (0.5 + 1.5 * rng.random(g.rows)).astype(np.float32)
    R = 777
    keep = g.row != R
    row = np.concatenate([g.row[keep], np.full(2, R, np.uint32)])
    col = np.concatenate([g.col[keep], np.array([17, 400], np.uint32)])
    val = np.concatenate([g.val[keep] * scale[g.row[keep]], np.array([1e-3, 1e-3], np.float32)])
    order = np.argsort(row, kind="stable")
    m = coo(pkg, g.rows, g.cols, row[order], col[order], val[order])
    k = 20
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    ids = np.array([R, 5, R, 19000], dtype=np.uint32)
    val_p, idx_p = eng.similar(ids)
    assert R not in idx_p[0].tolist(), "the constructed row is in its own top-k: the case shows nothing"
    assert 5 in idx_p[1].tolist() and 19000 in idx_p[3].tolist()
    val_x, idx_x = eng.similar(ids, exclude_self=True)
    assert np.array_equal(idx_x[0], idx_p[0]) and np.array_equal(bits(val_x[0]), bits(val_p[0]))
    assert np.array_equal(idx_x[2], idx_p[2]) and np.array_equal(bits(val_x[2]), bits(val_p[2]))
    e_val, e_idx = _without_self(val_p, idx_p, ids)
    assert np.array_equal(idx_x, e_idx) and np.array_equal(bits(val_x), bits(e_val))
    assert idx_x[1, k - 1] == 0 and val_x[1, k - 1] == 0.0 and 5 not in idx_x[1, :k - 1].tolist()
    # the plain lists are the oracle's
    layout = Layout(pkg, eng, m)
    xs, _ = _Rows(m).vectors(ids)
    oval, oidx = _oracle_lists(oracle, layout, xs, k)
    assert np.array_equal(idx_p, oidx) and np.array_equal(bits(val_p), bits(oval))
    eng.close()


def test_knn_graph(pkg, oracle):
    m, _ = _matrix(pkg, 20000, 1024, 51)
    k = 10
    val, idx = pkg.knn_graph(m, k, device=0)
    assert val.shape == (m.rows, k) and idx.shape == (m.rows, k)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k + 1, device=0)  # (the engine knn_graph builds: the same layout)
    layout = Layout(pkg, eng, m)
    eng.close()
    ids = np.arange(m.rows, dtype=np.uint32)
    xs, _ = _Rows(m).vectors(ids)
    oval, oidx = _oracle_lists(oracle, layout, xs, k + 1)
    e_val, e_idx = _without_self(oval, oidx, ids)
    bad = np.flatnonzero(np.any(idx != e_idx[:, :k], axis=1) | np.any(bits(val) != bits(e_val[:, :k]), axis=1))
    assert bad.size == 0, f"knn_graph differs from the oracle's top-{k + 1} without the row itself for rows {bad[:8]}"
    # a subset of rows
    sub = np.array([102, 5, TRIPLE, 19999, 5], dtype=np.uint32)
    sval, sidx = pkg.knn_graph(m, k, rows=sub, device=0)
    assert np.array_equal(sidx, e_idx[sub, :k]) and np.array_equal(bits(sval), bits(e_val[sub, :k]))


def test_errors(pkg):
    import torch
    m = pkg.generate_matrix(5000, 512, 20, "gamma", 61)
    d_ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_xs = torch.full((4 * 512,), FILL_X, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def status_of(fn):
        try:
            fn()
        except pkg.TkspmvError as e:
            return e.status
        return 0

    for prec in (pkg.F16, pkg.Q1_7_F32):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0, precision=prec)
        assert status_of(lambda: eng.enqueue_row_vectors(d_ids.data_ptr(), 4, d_xs.data_ptr())) == pkg._lib.ERR_UNSUPPORTED
        assert status_of(lambda: eng.row_vectors([0, 1])) == pkg._lib.ERR_UNSUPPORTED
        assert status_of(lambda: eng.similar([0, 1])) == pkg._lib.ERR_UNSUPPORTED
        eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=8, device=0)
    INVALID = pkg._lib.ERR_INVALID
    assert status_of(lambda: eng.enqueue_row_vectors(0, 4, d_xs.data_ptr())) == INVALID
    assert status_of(lambda: eng.enqueue_row_vectors(d_ids.data_ptr(), 4, 0)) == INVALID
    assert status_of(lambda: eng.enqueue_row_vectors(d_ids.data_ptr(), 0, d_xs.data_ptr())) == INVALID
    assert status_of(lambda: eng.enqueue_row_vectors(d_ids.data_ptr(), -3, d_xs.data_ptr())) == INVALID
    lib = pkg._lib.lib()
    assert lib.tkspmv_row_vectors(eng._h, None, 2, None, None) == INVALID
    assert lib.tkspmv_run_similar(eng._h, None, 2, 0, None, None) == INVALID
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.all(bits(d_xs.cpu().numpy()) == bits(np.float32(FILL_X))), "a rejected call wrote its output"
    # empty requests of the Python layer are answered without a call
    xs, ln = eng.row_vectors([])
    assert xs.shape == (0, 512) and ln.shape == (0,)
    v, i = eng.similar([])
    assert v.shape == (0, 8) and i.shape == (0, 8)
    eng.close()
