"""Launch paths that only an option or a measurement entry point reaches: the plain host path, the event bracket of tkspmv_run,
the staged upload of x, the unfused selection, the forced radix select, short batch launches, the trace and hand-over stamps, the
statistics hooks under tkspmv_profile, tkspmv_time_query_batches and a single chain of multi-query launches. Two shapes: S (20 000 x
512 x 12 uniform: the device-wide exchange, kernels with tracing twins) and L (300 000 x 1024 x 20 gamma: checked workgroup-local
thresholds). Every list is compared with the CPU gold and bit for bit with the order-matched oracle on the engine's own packing.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_single import _exact, _packed_raw

pytestmark = pytest.mark.gpu
K = 100


class _Shape:
    def __init__(self, pkg, rows, cols, nnz, dist, seed, n_q, x_seed):
        self.m = pkg.generate_matrix(rows, cols, nnz, dist, seed)
        self.xs = np.stack([pkg.create_sample_vector(cols, True, False, True, x_seed + i) for i in range(n_q)])
        self._raw = {}

    def engine(self, pkg, **kw):
        m = self.m
        return pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=K, device=0, **kw)

    def raw(self, pkg, eng):  # the engine's own packing, packed once per partition count
        info = eng.info()
        key = (info["packet_entries"], (info["batch_mode"] >> 16) or info["n_wave_partitions"])
        if key not in self._raw:
            self._raw[key] = _packed_raw(pkg, self.m, eng, K)
        return self._raw[key]

    def exact(self, pkg, oracle, eng, q, idx, val):
        _, raw, c = self.raw(pkg, eng)
        _exact(pkg, oracle, self.m, eng, self.xs[q], K, idx, val, raw, c)

    def batch(self, pkg, oracle, eng, n):
        """One enqueue_batch of the first n vectors with per-query buffers; every list exact."""
        import torch
        dxs = torch.from_numpy(np.ascontiguousarray(self.xs[:n])).cuda()
        out_i = torch.zeros(n, K, dtype=torch.int32, device="cuda")
        out_v = torch.zeros(n, K, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        bi, bv = out_i.cpu().numpy().astype(np.uint32), out_v.cpu().numpy()
        for q in range(n):
            self.exact(pkg, oracle, eng, q, bi[q], bv[q])


@pytest.fixture(scope="module")
def S(pkg):
    return _Shape(pkg, 20000, 512, 12, "uniform", 11, 40, 5000)


@pytest.fixture(scope="module")
def L(pkg):
    return _Shape(pkg, 300000, 1024, 20, "gamma", 7, 40, 6000)


def _trace(pkg, eng, words):
    """tkspmv_debug_trace into a buffer a little longer than `words`: the stamps, and how many words the engine returned."""
    buf = np.zeros(words + 64, dtype=np.uint64)
    got = C.c_uint64()
    pkg._lib.check(pkg._lib.lib().tkspmv_debug_trace(eng._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size, C.byref(got)))
    return buf, int(got.value)


@pytest.mark.parametrize("option", ["HOST_PATH=0", "RUN_EVENTS=1", "BAR_X=0", "FUSED=0", "RADIX=1"])
def test_reference_loop_and_a_batch_under_an_option_that_changes_the_launch_path(pkg, oracle, monkeypatch, S, option):
    name, value = option.split("=")
    monkeypatch.setenv("TKSPMV_" + name, value)
    eng = S.engine(pkg)
    for q in range(6):
        eng.reset(S.xs[q])
        assert eng() > 0
        val, idx = eng.read_result()
        S.exact(pkg, oracle, eng, q, idx, val)
    S.batch(pkg, oracle, eng, 40)
    eng.close()


def test_batch_max_cuts_a_batch_into_short_launches(pkg, oracle, monkeypatch, L):
    monkeypatch.setenv("TKSPMV_BATCH_MAX", "5")
    eng = L.engine(pkg)
    assert (eng.info()["batch_mode"] >> 8) & 0xFF, "this size is expected to stream with workgroup-local thresholds"
    before = eng.debug_counters()["batch_launches"]
    L.batch(pkg, oracle, eng, 23)
    assert eng.debug_counters()["batch_launches"] == before + 5
    eng.close()


def test_trace_of_the_last_four_launches(pkg, oracle, monkeypatch, S):
    monkeypatch.setenv("TKSPMV_TRACE", "1")
    eng = S.engine(pkg)
    for q in range(3):
        eng.reset(S.xs[q])
        eng()
        val, idx = eng.read_result()
        S.exact(pkg, oracle, eng, q, idx, val)
    words = 4 * (eng.info()["grid"] + 1) * 72
    buf, got = _trace(pkg, eng, words)
    assert got == words and buf.any()
    eng.close()


def test_hand_over_stamps_of_the_last_batch_launch(pkg, oracle, monkeypatch, L):
    monkeypatch.setenv("TKSPMV_WG_TIMES", "1")
    eng = L.engine(pkg)
    assert (eng.info()["batch_mode"] >> 8) & 0xFF
    L.batch(pkg, oracle, eng, 32)
    words = 33 * eng.info()["grid"]
    buf, got = _trace(pkg, eng, words)
    assert got == words and buf.any()
    eng.close()


def test_profile_with_the_statistics_hooks_then_a_query(pkg, oracle, monkeypatch, S):
    import torch
    monkeypatch.setenv("TKSPMV_STATS", "1")
    monkeypatch.setenv("TKSPMV_STAMPS", "1")
    eng = S.engine(pkg)
    dxs = torch.from_numpy(np.ascontiguousarray(S.xs[:5])).cuda()
    torch.cuda.synchronize()
    t = eng.profile(dxs.data_ptr(), 5, 20)
    assert t["query_ns"] > 0 and t["stream_kernel_ns"] > 0 and t["scores_kernel_ns"] > 0, t
    eng.reset(S.xs[7])
    eng()
    val, idx = eng.read_result()
    S.exact(pkg, oracle, eng, 7, idx, val)
    eng.close()


def test_time_query_batches_leaves_the_last_query_in_the_engine_buffers(pkg, oracle, L):
    import torch
    eng = L.engine(pkg)
    dxs = torch.from_numpy(np.ascontiguousarray(L.xs[:7])).cuda()
    torch.cuda.synchronize()
    ns = eng.time_query_batches(dxs.data_ptr(), 7, 40, 3)
    assert len(ns) == 3 and all(v > 0 for v in ns), ns
    val, idx = eng.read_result()
    L.exact(pkg, oracle, eng, (40 - 1) % 7, idx, val)
    eng.close()


def test_multi_query_launches_on_a_single_chain(pkg, oracle, monkeypatch):
    """The engine of test_multi_query_passes_are_bit_identical_to_the_gold_order (4 queries per pass), its second chain switched
    off: every list equals the exact selection over the scores in that kernel's summation order."""
    import torch
    monkeypatch.setenv("TKSPMV_MULTI_CHAINS", "1")
    n_q = 40
    m = pkg.generate_matrix(70000, 1024, 20, "gamma", 77)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 300 + i) for i in range(n_q)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=K, device=0, stream_replicas=2, multi_q=4)
    assert eng.info()["multi_q"] == 4
    out_i = torch.full((n_q, K), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((n_q, K), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_multi(dxs.data_ptr(), n_q, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    bi, bv = out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy()
    for q in range(n_q):
        y, present = oracle.scores_f32_segmented(m.row, m.col, m.val, xs[q], m.rows)
        ei, ev = oracle.select_topk(y, present, K)
        assert np.array_equal(bi[q], ei), q
        assert np.array_equal(bv[q].view(np.uint32), ev.view(np.uint32)), q
    eng.close()
