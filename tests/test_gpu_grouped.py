"""Grouped top-k (tkspmv_set_groups / tkspmv_enqueue_grouped / tkspmv_run_grouped) on the MI355X.

Every result is compared EXACTLY -- row ids, score bits, group ids, the count -- with collapse_topk (host.py), the numpy restatement
of the contract whose ordering tests/test_grouped_host.py pins to the oracle's selection. The scores it collapses are the
order-matched oracle's over the engine's own layout for fp32 engines, and the engine's own full score vector (eng.scores()) for the
other value types. The conftest syncs torch only for the older enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import EngineSetup, GuardedOut, Scores, status_of

pytestmark = pytest.mark.gpu

PAD_GROUP = 0xFFFFFFFF


class _Out(GuardedOut):
    """[count][k] device outputs for idx / val / grp and [count] for n, each between two guard zones."""
    COLUMNS = (("dev_idx", "k", "int32"), ("dev_val", "k", "float32"), ("dev_grp", "k", "int32"), ("dev_n", 1, "int32"))

    def read(self):
        """(idx[count, k] uint32, val[count, k] float32, grp[count, k] uint32, n[count]); the guard zones must be untouched."""
        res = super().read()
        return res["dev_idx"].view(np.uint32), res["dev_val"], res["dev_grp"].view(np.uint32), res["dev_n"][:, 0]


def _same(got, want, what=""):
    idx, val, grp, n = got
    ei, ev, eg, en = want
    assert int(n) == en, (what, int(n), en)
    assert np.array_equal(idx, ei), (what, "row ids differ from collapse_topk")
    assert np.array_equal(val.view(np.uint32), ev.view(np.uint32)), (what, "scores are not bit-identical")
    assert np.array_equal(grp, eg), (what, "group ids differ")
    assert np.all(idx[en:] == 0) and np.all(val[en:].view(np.uint32) == 0) and np.all(grp[en:] == PAD_GROUP), (what, "pads")


def _query(eng, torch, dxs, count, stream=0, **kw):
    """enqueue_grouped into fresh guarded buffers; waits; [(idx, val, grp, n)] per query."""
    out = _Out(torch, count, eng.k)
    torch.cuda.synchronize()
    eng.enqueue_grouped(dxs.data_ptr() if dxs is not None else 0, count, stream=stream.cuda_stream if stream else 0, **out.ptrs(), **kw)
    if stream:
        stream.synchronize()
    else:
        eng.synchronize()
    idx, val, grp, n = out.read()
    return [(idx[q], val[q], grp[q], n[q]) for q in range(count)]


def _labelings(rows, seed):
    rng = np.random.default_rng(seed)
    ends = np.cumsum(rng.integers(1, 201, rows))  # runs of 1..200 rows: they start and end mid-wave and span up to three waves
    runs = np.searchsorted(ends, np.arange(rows), side="right")
    return {
        "identity": (np.arange(rows), rows),
        "runs": (runs, int(runs.max()) + 1),
        "mod2": (np.arange(rows) % 2, 2),
        "mod997": (np.arange(rows) % 997, 997),
        "one": (np.zeros(rows, dtype=np.int64), 1),
        "sparse": (rng.choice(3 * rows, rows, replace=False), 3 * rows),  # most groups have no row at all
        "forty": (rng.integers(0, 40, rows), 40),                         # fewer groups than k: pads, n, 0xFFFFFFFF
    }


LABELINGS = ("identity", "runs", "mod2", "mod997", "one", "sparse", "forty")
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
}


class _Setup(EngineSetup):
    """The engine and scores of one of CONFIGS, and the labelings of its rows; the expectation collapses the scores."""
    def __init__(self, pkg, oracle, torch, name):
        super().__init__(pkg, oracle, torch, CONFIGS[name])
        self.labelings = _labelings(self.m.rows, self.m.rows + 1)

    def expect(self, pkg, labels, allow=None, y=None, present=None):
        y = self.y if y is None else y
        present = self.present if present is None else present
        return pkg.collapse_topk(y, present if allow is None else present & allow, labels, self.k, self.min_score, self.first_row)


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request, pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, request.param)
    yield s
    s.eng.close()


@pytest.mark.parametrize("labeling", LABELINGS)
def test_grouped_matches_collapse_topk(pkg, setup, labeling):
    import torch
    s, eng = setup, setup.eng
    labels, n_groups = s.labelings[labeling]
    eng.set_groups(labels, n_groups)
    want = s.expect(pkg, labels)
    got, = _query(eng, torch, s.dx, 1)
    _same(got, want, labeling)
    # the host form: the installed vector, cut to the real entries
    val, idx, grp = eng.run_grouped()
    n = want[3]
    assert idx.size == n and np.array_equal(idx, want[0][:n]) and np.array_equal(val.view(np.uint32), want[1][:n].view(np.uint32)) and np.array_equal(grp, want[2][:n])
    if labeling == "identity":
        assert np.array_equal(got[2][:n], got[0][:n] - s.first_row), "group ids must be the local rows"
        if s.fp32:  # one row per group: the same engine's exact top-k, bit for bit
            fv, fi = eng.run_filtered(allow=np.ones(s.m.rows, dtype=bool))
            assert np.array_equal(fi, got[0]) and np.array_equal(fv.view(np.uint32), got[1].view(np.uint32))
    if labeling == "one":
        assert n == 1 and got[0][0] == want[0][0]
    if labeling == "forty" and s.min_score == 0.0:
        assert n == 40 < s.k
    if labeling == "mod2" and s.min_score == 0.0:
        assert n == 2


@pytest.fixture(scope="module")
def plain(pkg, oracle):
    import torch
    s = _Setup(pkg, oracle, torch, "default12bit")
    yield s
    s.eng.close()


def test_ties_within_groups_and_across_the_cut(pkg, oracle):
    import torch
    rows, cols, k = 20011, 1024, 100
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 31)
    m.val = np.ones_like(m.val)  # all ones and a vector of small integers: integer scores, exact in any order, tied everywhere
    x = np.random.default_rng(2).integers(0, 3, cols).astype(np.float32)
    eng = pkg.SpMV(m.row, m.col, m.val, rows, cols, k=k, device=0)
    y, present = Scores(pkg, eng, m)(oracle, x)
    assert np.unique(y[present]).size < 200
    labels = np.arange(rows) // 7
    eng.set_groups(labels)
    want = pkg.collapse_topk(y, present, labels, k)
    assert y[want[0][k - 1]] == y[want[0][k - 2]], "the cut must fall inside a tie for this test to mean anything"
    got, = _query(eng, torch, torch.from_numpy(x).cuda(), 1)
    _same(got, want, "ties")
    eng.close()


def test_masks(pkg, oracle, plain):
    import torch
    s, eng, rows = plain, plain.eng, plain.m.rows
    labels, n_groups = s.labelings["runs"]
    eng.set_groups(labels, n_groups)
    rng = np.random.default_rng(8)
    for density in (0.5, 0.001):
        allow = rng.random(rows) < density
        dmask = torch.from_numpy(pkg.row_mask(rows, allow).view(np.int32)).cuda()
        got, = _query(eng, torch, s.dx, 1, dev_mask=dmask.data_ptr())
        _same(got, s.expect(pkg, labels, allow), f"mask {density}")
    # a mask per query, with a stride: 3 queries, 3 masks
    xs = np.stack([pkg.create_sample_vector(s.m.cols, True, False, True, 70 + i) for i in range(3)]).astype(np.float32)
    allows = [rng.random(rows) < d for d in (0.5, 0.02, 0.9)]
    words = np.stack([pkg.row_mask(rows, a) for a in allows])
    dmask = torch.from_numpy(words.view(np.int32)).cuda()
    got = _query(eng, torch, torch.from_numpy(xs).cuda(), 3, dev_mask=dmask.data_ptr(), mask_stride=words.shape[1])
    for q in range(3):
        y, present = s.scores(oracle, xs[q])
        _same(got[q], s.expect(pkg, labels, allows[q], y, present), f"per-query mask {q}")
    # every representative of the unmasked answer masked out: the groups come back by their next-best row
    free = s.expect(pkg, labels)
    removed = free[0][:free[3]].astype(np.int64) - s.first_row
    allow = np.ones(rows, dtype=bool)
    allow[removed] = False
    want = s.expect(pkg, labels, allow)
    dmask = torch.from_numpy(pkg.row_mask(rows, allow).view(np.int32)).cuda()  # (kept alive: the query reads it)
    got, = _query(eng, torch, s.dx, 1, dev_mask=dmask.data_ptr())
    _same(got, want, "representatives removed")
    assert not set(got[0][:got[3]].tolist()) & set((removed + s.first_row).tolist())
    assert len(set(got[2][:got[3]].tolist()) & set(free[2][:free[3]].tolist())) > 0, "groups with a second eligible row must come back"
    # the host form with the installed mask
    val, idx, grp = eng.run_grouped(allow=allow)
    assert np.array_equal(idx, want[0][:want[3]]) and np.array_equal(grp, want[2][:want[3]])
    eng.set_filter(None)


def test_sequence_on_a_callers_stream_is_reproducible(pkg, oracle, plain):
    import torch
    s, eng = plain, plain.eng
    labels, n_groups = s.labelings["runs"]
    eng.set_groups(labels, n_groups)
    xs = np.stack([pkg.create_sample_vector(s.m.cols, True, False, True, 90 + i) for i in range(5)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    side = torch.cuda.Stream()
    first = _query(eng, torch, dxs, 5, stream=side)
    second = _query(eng, torch, dxs, 5, stream=side)
    for q in range(5):
        y, present = s.scores(oracle, xs[q])
        _same(first[q], s.expect(pkg, labels, None, y, present), f"query {q}")
        for a, b in zip(first[q][:3], second[q][:3]):  # the same call again: identical bits (the per-group keys were reset)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert first[q][3] == second[q][3]


def test_no_cross_talk_with_the_batch_path(pkg, oracle, plain):
    import torch
    s, eng, k = plain, plain.eng, plain.k
    labels, n_groups = s.labelings["mod997"]
    eng.set_groups(labels, n_groups)
    nq = 40
    xs = np.stack([pkg.create_sample_vector(s.m.cols, True, False, True, 200 + i) for i in range(nq)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    b_i = [torch.zeros((nq, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    b_v = [torch.zeros((nq, k), dtype=torch.float32, device="cuda") for _ in range(2)]
    out = _Out(torch, 2, k)
    torch.cuda.synchronize()
    # an unwaited batch sequence, the grouped call right behind it, another batch sequence right behind that: one stream, one wait
    eng.enqueue_batch(dxs.data_ptr(), nq, b_i[0].data_ptr(), b_v[0].data_ptr())
    eng.enqueue_grouped(dxs.data_ptr() + 4 * 7 * s.m.cols, 2, **out.ptrs())  # queries 7 and 8
    eng.enqueue_batch(dxs.data_ptr(), nq, b_i[1].data_ptr(), b_v[1].data_ptr())
    eng.synchronize()
    scores = [s.scores(oracle, xs[q]) for q in range(nq)]
    for q in range(nq):
        ei, ev = oracle.select_topk(scores[q][0], scores[q][1].astype(np.uint8), k)
        for j in range(2):
            assert np.array_equal(b_i[j][q].cpu().numpy().view(np.uint32), ei), (j, q)
            assert np.array_equal(b_v[j][q].cpu().numpy().view(np.uint32), ev.view(np.uint32)), (j, q)
    idx, val, grp, n = out.read()
    for j, q in enumerate((7, 8)):
        _same((idx[j], val[j], grp[j], n[j]), s.expect(pkg, labels, None, *scores[q]), f"grouped query {q}")
    before = eng.debug_counters()
    # engine-owned outputs: tkspmv_read returns the grouped list (the last query wins), pads included
    torch.cuda.synchronize()
    eng.enqueue_grouped(dxs.data_ptr(), 3)
    eng.synchronize()
    rv, ri = eng.read_result()
    want = s.expect(pkg, labels, None, *scores[2])
    assert np.array_equal(ri, want[0]) and np.array_equal(rv.view(np.uint32), want[1].view(np.uint32))
    eng.reset(xs[11])
    val, idx, grp = eng.run_grouped()
    want = s.expect(pkg, labels, None, *scores[11])
    assert np.array_equal(idx, want[0][:want[3]]) and np.array_equal(grp, want[2][:want[3]])
    rv, ri = eng.read_result()
    assert np.array_equal(ri, want[0]) and np.array_equal(rv.view(np.uint32), want[1].view(np.uint32))
    after = eng.debug_counters()
    for key in ("checks_failed", "late_repairs", "single_repairs", "single_checks_failed", "batch_launches", "single_launches"):
        assert after[key] == before[key], (key, before, after)  # the grouped calls ran no batch or single launch and failed no check
    # ... and the batch path still answers exactly behind them
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), nq, b_i[0].data_ptr(), b_v[0].data_ptr())
    eng.synchronize()
    ei, ev = oracle.select_topk(scores[nq - 1][0], scores[nq - 1][1].astype(np.uint8), k)
    assert np.array_equal(b_i[0][nq - 1].cpu().numpy().view(np.uint32), ei)
    eng.reset(s.x)


def test_errors(pkg, oracle):
    import torch
    L = pkg._lib
    m = pkg.generate_matrix(20011, 1024, 20, "gamma", 4)
    x = pkg.create_sample_vector(1024, True, False, True, 2)
    rows, k = m.rows, 100
    labels = np.arange(rows) // 5
    dmask = torch.from_numpy(pkg.row_mask(rows).view(np.int32)).cuda()
    buf = torch.zeros(k, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0)
    eng.reset(x)
    assert status_of(pkg, eng.enqueue_grouped, 0, 1) == L.ERR_STATE  # before set_groups
    assert status_of(pkg, eng.run_grouped) == L.ERR_STATE
    assert status_of(pkg, eng.set_groups, labels, int(labels.max())) == L.ERR_INVALID  # a label == n_groups ...
    assert status_of(pkg, eng.enqueue_grouped, 0, 1) == L.ERR_STATE                     # ... installs nothing
    assert status_of(pkg, eng.set_groups, labels, 0) == L.ERR_INVALID
    eng.set_groups(labels)
    val, idx, grp = eng.run_grouped()
    assert status_of(pkg, eng.set_groups, labels + 1, int(labels.max()) + 1) == L.ERR_INVALID  # the labels installed before stay
    v2, i2, g2 = eng.run_grouped()
    assert np.array_equal(i2, idx) and np.array_equal(g2, grp) and np.array_equal(v2.view(np.uint32), val.view(np.uint32))
    assert status_of(pkg, eng.enqueue_grouped, 0, 0) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_grouped, 0, 1, dmask.data_ptr(), -1) == L.ERR_INVALID
    for given in ((1, 0, 0), (1, 1, 0), (0, 1, 1), (0, 0, 1)):  # output pointers partly given
        p = [buf.data_ptr() if g else 0 for g in given]
        assert status_of(pkg, eng.enqueue_grouped, 0, 1, 0, 0, *p) == L.ERR_INVALID
    n = C.c_int32(0)
    assert L.lib().tkspmv_run_grouped(eng._h, 1, None, None, None, C.byref(n)) == L.ERR_INVALID  # use_filter, none installed
    eng.set_groups(None)
    assert status_of(pkg, eng.enqueue_grouped, 0, 1) == L.ERR_STATE  # removed
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0)
    eng.set_groups(labels)
    assert status_of(pkg, eng.enqueue_grouped, 0, 1) == L.ERR_STATE    # no query vector installed
    assert status_of(pkg, eng.enqueue_grouped, 0, 2) == L.ERR_INVALID  # NULL dev_xs takes the installed vector: count must be 1
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0, partitions=4, k_per_partition=8)  # the approximate per-partition path
    eng.reset(x)
    eng.set_groups(labels)
    assert status_of(pkg, eng.run_grouped) == L.ERR_UNSUPPORTED
    eng.close()
    eng = pkg.SpMV(m.row, m.col, m.val, rows, 1024, k=k, device=0, precision=pkg.F16)
    eng.reset(x)
    eng.set_groups(labels)
    eng.run_grouped()  # served without a mask ...
    assert status_of(pkg, eng.enqueue_grouped, 0, 1, dmask.data_ptr()) == L.ERR_UNSUPPORTED  # ... a mask needs the filter kernels
    with pytest.raises(pkg.TkspmvError) as e:
        eng.enqueue_grouped(0, 1, dmask.data_ptr())
    assert "filtered queries need fp32 values" in str(e.value)
    eng.close()
