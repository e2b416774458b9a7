"""The shard merge (merge_kernel of csrc/dist.hip behind tkspmv_merge_topk, tkspmv_merge_topk_batch and tkspmv_dist_*) on short,
signed and tied lists, bit for bit against the plain numpy reference of tests/merge_ref.py.

  * synthetic buffers: the case table of merge_ref.py and the sizes at the LDS limit, through the single and the batch entry
    (a different case per query, so a wrong [world][n_q][2][k] stride shows), outputs prefilled with a sentinel; the refusals;
  * real shard engines over a small signed matrix cut so that one shard is shorter than k and one has a single row: per-shard
    lists against the order-matched oracle, the merged list against merge_reference over the oracle's lists (n_real = what the
    oracle's selection found eligible) and, independently, against float64 scores of the whole matrix within a derived bound;
  * the pipelined step with one rank on the short shard: every list is the engine's own;
  * a shard without entries is refused by tkspmv_create."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import merge_ref

pytestmark = pytest.mark.gpu
SENTINEL = 0x5EA7BEEF  # (as float32 bits: a finite value no case produces; as a row id: outside every case's rows)
SLACK = 64             # sentinel words behind the n_q * k entries a merge may write
TABLE = merge_ref.table()
SIZES = [(8, 1023), (7, 1024), (1, 1024), (2, 8)]  # (8, 1023) = 8184 = the limit, where the dynamic LDS is exactly 64 KiB


@pytest.fixture(scope="module")
def dmod(pkg):
    return import_module("approximate_spmv_topk_amd.distributed")


def _outputs(torch, n):
    out_i = torch.full((n + SLACK,), SENTINEL, dtype=torch.int32, device="cuda")
    out_v = torch.full((n + SLACK,), SENTINEL, dtype=torch.int32, device="cuda")
    return out_i, out_v


def _check_written(cases, out_i, out_v):
    """Exactly n_q * k entries were written, and every one is the reference's, as bits."""
    k = cases[0]["k"]
    n = len(cases) * k
    got_i, got_v = out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy().view(np.uint32)
    assert np.all(got_i[n:] == SENTINEL) and np.all(got_v[n:] == SENTINEL), "the merge wrote behind its n_q * k entries"
    for q, c in enumerate(cases):
        want_i, want_v = merge_ref.expected(c)
        assert np.array_equal(got_i[q * k:(q + 1) * k], want_i), (c["name"], q, got_i[q * k:(q + 1) * k][:12], want_i[:12])
        assert np.array_equal(got_v[q * k:(q + 1) * k], want_v.view(np.uint32)), (c["name"], q)
    return got_i, got_v


def _merge_single(pkg, torch, case):
    gt = torch.from_numpy(merge_ref.gathered([case])).cuda()
    out_i, out_v = _outputs(torch, case["k"])
    torch.cuda.synchronize()
    pkg._lib.check_dist(pkg._lib.lib().tkspmv_merge_topk(C.c_void_p(gt.data_ptr()), case["world"], case["k"], C.c_void_p(out_i.data_ptr()),
                                                         C.c_void_p(out_v.data_ptr()), C.c_void_p(0)))
    torch.cuda.synchronize()
    return gt, out_i, out_v


def _merge_batch(pkg, torch, cases):
    world, k = cases[0]["world"], cases[0]["k"]
    gt = torch.from_numpy(merge_ref.gathered(cases)).cuda()
    out_i, out_v = _outputs(torch, len(cases) * k)
    torch.cuda.synchronize()
    pkg._lib.check_dist(pkg._lib.lib().tkspmv_merge_topk_batch(C.c_void_p(gt.data_ptr()), world, len(cases), k, C.c_void_p(out_i.data_ptr()),
                                                               C.c_void_p(out_v.data_ptr()), C.c_void_p(0)))
    torch.cuda.synchronize()
    return gt, out_i, out_v


_SIZE_CASES = {}


def _size_case(world, k):
    if (world, k) not in _SIZE_CASES:
        _SIZE_CASES[(world, k)] = merge_ref.random_case(world, k, seed=7 * world + k)
    return _SIZE_CASES[(world, k)]


def _all_cases():
    return TABLE + [_size_case(w, k) for w, k in SIZES]


def _ids():
    return [c["name"] for c in TABLE] + [f"size_w{w}_k{k}" for w, k in SIZES]


@pytest.mark.parametrize("i", range(len(TABLE) + len(SIZES)), ids=_ids())
def test_merge_topk_against_the_reference(pkg, dmod, i):
    """tkspmv_merge_topk on one case: the reference's list as bits, nothing written behind it, and merge_candidates on the same
    device tensors agrees with the kernel."""
    import torch
    case = _all_cases()[i]
    gt, out_i, out_v = _merge_single(pkg, torch, case)
    got_i, got_v = _check_written([case], out_i, out_v)
    k = case["k"]
    idx = gt[:, 0, 0, :].reshape(-1).to(torch.int64) & 0xFFFFFFFF
    val = gt[:, 0, 1, :].reshape(-1).contiguous().view(torch.float32)
    ei, ev = dmod.merge_candidates(idx, val, k)
    assert np.array_equal(ei.cpu().numpy().astype(np.uint32), got_i[:k])
    assert np.array_equal(ev.cpu().numpy().view(np.uint32), got_v[:k])


@pytest.mark.parametrize("n_q", [1, 2, 32])
@pytest.mark.parametrize("i", range(len(TABLE) + len(SIZES)), ids=_ids())
def test_merge_topk_batch_against_the_reference(pkg, dmod, i, n_q):
    """tkspmv_merge_topk_batch: the case in one slot of the batch, a different random case of the same (world, k) in every other."""
    import torch
    case = _all_cases()[i]
    cases = [merge_ref.random_case(case["world"], case["k"], seed=1000 + q) for q in range(n_q)]
    cases[n_q // 2] = case
    gt, out_i, out_v = _merge_batch(pkg, torch, cases)
    got_i, got_v = _check_written(cases, out_i, out_v)
    k = case["k"]
    for q in sorted({0, n_q // 2, n_q - 1}):  # merge_candidates agrees with the kernel, list for list
        idx = gt[:, q, 0, :].reshape(-1).to(torch.int64) & 0xFFFFFFFF
        val = gt[:, q, 1, :].reshape(-1).contiguous().view(torch.float32)
        ei, ev = dmod.merge_candidates(idx, val, k)
        assert np.array_equal(ei.cpu().numpy().astype(np.uint32), got_i[q * k:(q + 1) * k])
        assert np.array_equal(ev.cpu().numpy().view(np.uint32), got_v[q * k:(q + 1) * k])


def test_merge_refusals_leave_the_outputs_alone(pkg):
    """world * k > 8184, world = 0, k = 0, n_q = 0, n_q = 33 and a NULL pointer: TKSPMV_ERR_INVALID, nothing launched."""
    import torch
    lib, INVALID = pkg._lib.lib(), pkg._lib.ERR_INVALID
    gt = torch.zeros(8 * 33 * 2 * 1024, dtype=torch.int32, device="cuda")
    out_i, out_v = _outputs(torch, 33 * 1024)
    torch.cuda.synchronize()
    g, oi, ov, null = C.c_void_p(gt.data_ptr()), C.c_void_p(out_i.data_ptr()), C.c_void_p(out_v.data_ptr()), C.c_void_p(0)
    assert lib.tkspmv_merge_topk(g, 8, 1024, oi, ov, null) == INVALID
    assert "world * k must be <= 8184" in lib.tkspmv_dist_last_error().decode()
    assert lib.tkspmv_merge_topk(g, 0, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk(g, 2, 0, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk(g, -1, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk(null, 2, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk(g, 2, 100, null, ov, null) == INVALID
    assert lib.tkspmv_merge_topk(g, 2, 100, oi, null, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(g, 8, 1, 1024, oi, ov, null) == INVALID
    assert "world * k must be <= 8184" in lib.tkspmv_dist_last_error().decode()
    assert lib.tkspmv_merge_topk_batch(g, 0, 4, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(g, 2, 4, 0, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(g, 2, 0, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(g, 2, 33, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(null, 2, 4, 100, oi, ov, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(g, 2, 4, 100, null, ov, null) == INVALID
    assert lib.tkspmv_merge_topk_batch(g, 2, 4, 100, oi, null, null) == INVALID
    torch.cuda.synchronize()
    assert bool((out_i == SENTINEL).all()) and bool((out_v == SENTINEL).all())


def test_dist_create_refuses_world_times_k_above_the_limit(pkg, monkeypatch):
    """world = 8 with an engine of k = 1024 is refused (8192 > 8184) with a message that states the limit; k = 1023 is accepted.
    TKSPMV_DIST_NO_NCCL: no communicator is attempted."""
    monkeypatch.setenv("TKSPMV_DIST_NO_NCCL", "1")
    lib = pkg._lib.lib()
    m = pkg.generate_matrix(3000, 128, 8, "uniform", 1)
    for k, want in ((1024, pkg._lib.ERR_INVALID), (1023, pkg._lib.OK)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
        h = C.c_void_p()
        assert lib.tkspmv_dist_create(C.byref(h), eng._h, None, 0, 8) == want
        if want == pkg._lib.OK:
            assert h.value
            lib.tkspmv_dist_destroy(h)
        else:
            assert not h.value and "world * k must be <= 8184" in lib.tkspmv_dist_last_error().decode()
        eng.close()


# ---- real shard engines ----------------------------------------------------------------------------------------------------
K = 100
BOUNDS = [(0, 37), (37, 1500), (1500, 1501), (1501, 3000)]  # one shard shorter than k, one of a single row
N_Q = 6


@pytest.fixture(scope="module")
def signed(pkg, oracle):
    m = merge_ref.signed_matrix(pkg)
    xs = np.stack([pkg.create_sample_vector(m.cols, True, False, True, 500 + i) for i in range(N_Q + 1)])
    # the independent leg: float64 scores of the whole matrix and, per row, b(r) = (len(r) + 1) * 2^-24 * sum |a_i * x_i|
    y64, bound = [], []
    for x in xs:
        y, present = oracle.scores_f64(m.row, m.col, m.val, x, m.rows)
        assert np.all(present != 0)
        sum_abs = np.zeros(m.rows, np.float64)
        np.add.at(sum_abs, m.row, np.abs(m.val.astype(np.float64) * x.astype(np.float64)[m.col]))
        length = np.bincount(m.row, minlength=m.rows).astype(np.float64)
        y64.append(y)
        bound.append((length + 1.0) * 2.0 ** -24 * sum_abs)
    return m, xs, y64, bound


@pytest.mark.parametrize("min_score", [-1e30, 0.0, 0.05])
def test_short_signed_shards_lists_and_merge(pkg, oracle, dmod, signed, min_score):
    import torch
    m, xs, y64, bound = signed
    world = len(BOUNDS)
    dxs = torch.from_numpy(xs[:N_Q]).cuda()
    local = torch.zeros(world, N_Q, 2, K, dtype=torch.int32, device="cuda")
    want = [[None] * world for _ in range(N_Q)]  # per query and shard: (idx, val, n_real) of the order-matched oracle
    y_all = [[None] * world for _ in range(N_Q)]
    for r, (r0, r1) in enumerate(BOUNDS):
        shard = merge_ref.shard_of(pkg, m, r0, r1)
        eng = pkg.SpMV(shard.row, shard.col, shard.val, shard.rows, shard.cols, k=K, device=0, first_row=r0, min_score=min_score)
        out_i = torch.full((N_Q, K), SENTINEL, dtype=torch.int32, device="cuda")
        out_v = torch.full((N_Q, K), SENTINEL, dtype=torch.int32, device="cuda")
        eng.enqueue_batch(dxs.data_ptr(), N_Q, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        local[r, :, 0, :] = out_i
        local[r, :, 1, :] = out_v
        got_i, got_v = out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy().view(np.uint32)
        for q in range(N_Q):
            y, present = merge_ref.shard_oracle_scores(pkg, oracle, shard, xs[q], K, eng)
            want[q][r] = merge_ref.shard_oracle_list(oracle, y, present, K, min_score, r0)
            y_all[q][r] = (y, present)
            # every shard's own list: the order-matched oracle's, ids with first_row, bits
            assert np.array_equal(got_i[q], want[q][r][0]) and np.array_equal(got_v[q], want[q][r][1].view(np.uint32)), (r, q)
        eng.close()
    assert want[0][0][2] <= 37 < K and want[0][2][2] <= 1  # the short shards do end in fillers
    torch.cuda.synchronize()
    mi, mv = dmod.merge_topk_batch_device(local.reshape(-1), world, N_Q, K)
    torch.cuda.synchronize()
    mi, mv = mi.cpu().numpy().view(np.uint32), mv.cpu().numpy()
    for q in range(N_Q):
        # bit-exact leg: merge_reference over the per-shard oracle lists ...
        ei, ev = merge_ref.merge_reference([(w[0], w[1]) for w in want[q]], [w[2] for w in want[q]], K)
        assert np.array_equal(mi[q], ei) and np.array_equal(mv[q].view(np.uint32), ev.view(np.uint32)), q
        # ... which is the selection over the concatenated per-shard scores
        si, sv = oracle.select_topk(np.concatenate([y for y, _ in y_all[q]]), np.concatenate([p for _, p in y_all[q]]), K, min_score)
        assert np.array_equal(ei, si) and np.array_equal(ev.view(np.uint32), sv.view(np.uint32)), q
        # independent leg: float64 scores of the whole matrix
        n_real = min(K, sum(int(np.count_nonzero((p != 0) & (y >= np.float32(min_score)))) for y, p in y_all[q]))
        assert n_real == K  # (half of 3000 signed rows score above 0.05: the lists are full)
        rows = mi[q][:n_real].astype(np.int64)
        err = np.abs(mv[q][:n_real].astype(np.float64) - y64[q][rows])
        print(f"min_score {min_score} query {q}: max |merged - f64| / b(r) = {np.max(err / bound[q][rows]):.3f}")
        assert np.all(err <= bound[q][rows]), q
        eligible = np.nonzero(y64[q] >= min_score)[0]
        top = eligible[np.argsort(-y64[q][eligible], kind="stable")[:K]]
        kth_row = top[-1]
        for r in set(rows.tolist()) ^ set(top.tolist()):
            assert abs(y64[q][r] - y64[q][kth_row]) <= bound[q][r] + bound[q][kth_row], (q, r)


def test_pipelined_step_on_the_short_shard_returns_the_engines_own_lists(pkg, dmod, signed):
    """One rank on the 37-row shard (k = 100: 63 fillers in every list), first_row = 5000, min_score = -1e30: every list the
    pipelined step returns is the engine's own read_result() for that query, bit for bit -- the fillers stay behind the negative
    scores."""
    import torch
    m, xs, _, _ = signed
    r0, r1 = BOUNDS[0]
    shard = merge_ref.shard_of(pkg, m, r0, r1)
    eng = pkg.SpMV(shard.row, shard.col, shard.val, shard.rows, shard.cols, k=K, device=0, first_row=5000, min_score=-1e30)
    own = []
    for q in range(7):
        eng.reset(xs[q])
        eng()
        val, idx = eng.read_result()
        assert np.all(idx[:37] >= 5000) and np.all(idx[37:] == 0) and np.all(val[37:].view(np.uint32) == 0) and np.any(val[:37] < 0)
        own.append((idx.copy(), val.copy()))
    dxs = torch.from_numpy(xs[:7]).cuda()
    torch.cuda.synchronize()
    nat = dmod.NativeShardedSpMV(eng, torch.device("cuda", 0))
    nat.set_batch(4)
    for q in range(7):
        nat.enqueue(dxs[q].data_ptr())
        if q in (2, 6):  # q = 2 flushes a partial batch; q = 6 closes the batch of queries 3..6
            val, idx = nat.read()
            assert np.array_equal(idx, own[q][0]) and np.array_equal(val.view(np.uint32), own[q][1].view(np.uint32)), q
    vb, ib = nat.read_batch()
    assert vb.shape[0] == 4
    for j in range(4):
        assert np.array_equal(ib[j], own[3 + j][0]) and np.array_equal(vb[j].view(np.uint32), own[3 + j][1].view(np.uint32)), j
    nat.close()
    eng.close()


def test_a_shard_without_entries_is_refused(pkg):
    """rows > 0, nnz = 0 (what shard_bounds_by_nnz can hand a rank): tkspmv_create refuses it; such a rank contributes k
    fillers to the merge (the all_fillers and random cases of the table) and needs no engine."""
    empty = np.zeros(0, np.uint32)
    with pytest.raises(pkg.TkspmvError) as e:
        pkg.SpMV(empty, empty, np.zeros(0, np.float32), 5, 128, k=K, device=0, first_row=1500)
    assert e.value.status == pkg._lib.ERR_INVALID and "no entries" in e.value.message
