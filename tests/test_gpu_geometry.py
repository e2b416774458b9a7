"""Launch geometries other than the default (512 workgroups of 8 streaming waves): SpMV(..., waves_per_cu=, threads_per_wg=).
tkspmv_create derives its gates from grid and block -- deferred selection and the fused tail (grid <= block + 64), the batch kernel,
the groups per workgroup, the radix path (k above 3/8 of the publishing groups), four selectors on small matrices (grid >= 64),
local thresholds and single_kernel (grid <= 512, block == 512) -- and the kernels derive their wave count from blockDim. Every
geometry below is a supported configuration; each case reads what the engine decided from info() and debug_counters(), asserts the
gate the geometry is meant to flip FROM THOSE VALUES (a device on which it does not flip fails the case and says so), and then runs
every entry point the geometry changes: tkspmv_run, enqueue_batch, enqueue_many, a filtered query, range queries, facet counts
(their kernels always launch 512 threads over the engine's grid and partition table) and score_rows.

Observed and inferred: info() reports grid, block, n_groups and batch_mode (selector workgroups of the batch kernel, 0 without it; the
mode of local thresholds), debug_counters() the launches of single_kernel and of the batch kernel. It has no word for the deferred
selection, the fused tail or the radix path: _gates()["defer"] and _radix() RESTATE create's rules from grid, block, k and n_groups,
so "served by radix" below is an inference (no batch kernel, no single_kernel, and the rule says radix), not an observation.
Not reached on a 256-CU device: the batch kernel with ONE streaming wave -- 64-thread workgroups make num_cus * waves_per_cu >= 256
workgroups, more than the block + 64 = 128 a deferred selection holds, so no geometry gets there; of the narrow workgroups only
384 x 9 and 256 x 4 run the batch kernel.

One matrix, 16 queries. Every top-k list is compared bit for bit with the order-matched oracle on the engine's own packing and
through _exact with the fp64 gold.
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import ctypes as C

import numpy as np
import pytest

from support import bits
from test_gpu_range import _Dev, _check_query, _expected
from test_gpu_single import _exact, _packed_raw

pytestmark = pytest.mark.gpu

COUNTERS = ("checks_failed", "single_launches", "single_repairs", "batch_launches", "late_repairs", "pace_period_ns")


class _Shape:
    """The matrix, its queries, and per partition count of an engine the re-packed stream and the oracle's scores of every query."""
    def __init__(self, pkg):
        self.m = pkg.generate_matrix(60000, 1024, 20, "gamma", 43)
        self.xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 900 + i) for i in range(16)]).astype(np.float32)
        rng = np.random.default_rng(43)
        self.allow = rng.random(self.m.rows) < 0.05
        self.ids = rng.choice(self.m.rows, 64, replace=False).astype(np.uint32)
        self.labels = np.arange(self.m.rows) % 37
        self._raw, self._scores = {}, {}

    def raw(self, pkg, eng):
        info = eng.info()
        key = (info["batch_mode"] >> 16) or info["n_wave_partitions"]
        if key not in self._raw:
            self._raw[key] = _packed_raw(pkg, self.m, eng, eng.k)
        assert self._raw[key][0].info()["n_wave_partitions"] == info["n_wave_partitions"]
        return key, self._raw[key][1], self._raw[key][2]

    def scores(self, pkg, oracle, eng, q):
        key, raw, c = self.raw(pkg, eng)
        if (key, q) not in self._scores:
            yp, present = oracle.packed_scores(raw, self.xs[q], self.m.rows, c)
            self._scores[(key, q)] = (yp, present.astype(bool))
        return self._scores[(key, q)]

    def exact(self, pkg, oracle, eng, q, idx, val):
        _, raw, c = self.raw(pkg, eng)
        _exact(pkg, oracle, self.m, eng, self.xs[q], eng.k, idx, val, raw, c)


@pytest.fixture(scope="module")
def shape(pkg):
    return _Shape(pkg)


def _engine(pkg, s, k, **kw):
    m = s.m
    return pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, **kw)


def _some(c):
    return {key: c[key] for key in COUNTERS}


def _gates(info):
    """batch / selectors / local / waves: read from info(). defer: setup_geometry's rule (grid <= block + 64) RESTATED from grid and
    block -- info() does not report the deferred selection; the cases use it to say which side of the rule a geometry lies on, and
    the observation that goes with it is whether the batch kernel (which needs the deferred selection) exists."""
    grid, block = info["grid"], info["block"]
    return dict(defer=grid >= 2 and grid <= block + 64, batch=info["batch_mode"] & 0xFF != 0, selectors=info["batch_mode"] & 0xFF,
                local=(info["batch_mode"] >> 8) & 0xFF, waves=block // 64)


def _batch(pkg, oracle, s, eng, n=16):
    import torch
    k = eng.k
    dxs = torch.from_numpy(np.ascontiguousarray(s.xs[:n])).cuda()
    out_i = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((n, k), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    bi, bv = out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy()
    for q in range(n):
        s.exact(pkg, oracle, eng, q, bi[q], bv[q])


def _every_entry_point(pkg, oracle, s, eng):
    """The checks of one geometry; returns which path served tkspmv_run and the counters behind the batch."""
    import torch
    k, rows = eng.k, s.m.rows
    c0 = eng.debug_counters()
    for q in range(4):
        eng.reset(s.xs[q])
        assert eng() > 0
        val, idx = eng.read_result()
        s.exact(pkg, oracle, eng, q, idx, val)
    c1 = eng.debug_counters()
    d = c1["single_launches"] - c0["single_launches"]
    assert d in (0, 4), f"{d} single_kernel launches for 4 tkspmv_run calls"
    _batch(pkg, oracle, s, eng)
    c2 = eng.debug_counters()
    dxs = torch.from_numpy(s.xs).cuda()
    torch.cuda.synchronize()
    eng.enqueue_many(dxs.data_ptr(), 16, 16)  # engine-owned result buffers: the last query wins
    eng.synchronize()
    val, idx = eng.read_result()
    s.exact(pkg, oracle, eng, 15, idx, val)
    # one filtered query under a 5 % mask
    yp, present = s.scores(pkg, oracle, eng, 0)
    dmask = torch.from_numpy(pkg.row_mask(rows, s.allow).view(np.int32)).cuda()
    out_i = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((k,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_filtered(dxs.data_ptr(), 1, dmask.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    ei, ev = oracle.select_topk(yp, (present & s.allow).astype(np.uint8), k)
    assert np.array_equal(out_i.cpu().numpy().view(np.uint32), ei), "filtered: index list differs from the order-matched oracle"
    assert np.array_equal(bits(out_v.cpu().numpy()), bits(ev)), "filtered: scores are not bit-identical"
    # range queries at the rank-10 and rank-1000 thresholds
    srt = np.sort(yp[present])[::-1]
    tv = np.array([srt[9], srt[999]], dtype=np.float32)
    ones = np.ones(rows, dtype=bool)
    exps = [_expected(yp, present, ones, t) for t in tv]
    cap = max(len(e) for e in exps)
    dev = _Dev(torch, 2, cap)
    dthr = torch.from_numpy(tv).cuda()
    dx2 = torch.from_numpy(np.tile(s.xs[0], (2, 1))).cuda()
    torch.cuda.synchronize()
    eng.enqueue_range(dx2.data_ptr(), 2, dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), cap)
    eng.synchronize()
    counts, gi, gv = dev.host()
    for i in range(2):
        _check_query(counts[i], gi[i], gv[i], cap, exps[i], f"range/{i}")
    # facet counts per label row % 37, score_rows of 64 rows
    fc, fbi, fbv, total = eng.run_facets(float(tv[1]), vec=s.xs[0], groups=s.labels)
    ec, ebi, ebv, et = pkg.facet_counts(yp, present, s.labels, 37, float(tv[1]))
    assert total == et and np.array_equal(fc, ec) and np.array_equal(fbi, ebi) and np.array_equal(bits(fbv), bits(ebv)), "facet counts differ"
    sc = eng.score_rows(s.ids, s.xs[0])
    assert np.array_equal(bits(sc[0]), bits(yp[s.ids])), "score_rows differs from the order-matched oracle"
    return ("single" if d == 4 else ("radix" if _radix(eng) else "stream")), c2  # ("radix": inferred, see the module's note)


def _radix(eng):
    """choose_path's rule restated (the exchange is off, or k above 3/8 of the publishing groups): what the engine SHOULD have chosen.
    info() does not report the choice itself."""
    info = eng.info()
    return info["n_groups"] == 0 or 8 * eng.k > 3 * info["n_groups"]


def _report(name, info, served, c):
    print(f"\n[{name}] grid {info['grid']} x block {info['block']}, n_groups {info['n_groups']}, batch_mode {info['batch_mode']:#x}, "
          f"n_wave_partitions {info['n_wave_partitions']} x {info['packets_per_partition']} packets; tkspmv_run served by {served}; {_some(c)}")


def _trace_and_timetable(pkg, oracle, monkeypatch, s, k, kw, name):
    """A narrow workgroup under TKSPMV_TRACE=1 (the stamps are laid out for 9 waves per workgroup: the call must return and the lists
    stay exact), then -- engines of local thresholds only: the kernel of the device-wide exchange keeps no timetable, so with
    TKSPMV_LOCAL=0 this leg is left out -- batches on the timetable WITH its adaptation. The period (TKSPMV_PACE_PERIOD) is what the
    engine reports or, since tkspmv_create does not tune engines of this size and they report none, what tkspmv_time_queries measures
    per query on the same engine. The adaptation's words (the late-wave count of the streaming waves, the selection's
    `n_waves = n_stream * 8u` adjustment) exist only on engines that pace by rank, which a matrix of under 25 000 packets does not by
    itself: TKSPMV_PACE=1 switches that on, and debug_counters() must say so. A launch of 16 queries (>= 8) runs the adjustment."""
    import torch
    monkeypatch.setenv("TKSPMV_TRACE", "1")
    eng = _engine(pkg, s, k, **kw)
    local = (eng.info()["batch_mode"] >> 8) & 0xFF
    eng.reset(s.xs[0])
    eng()
    val, idx = eng.read_result()
    s.exact(pkg, oracle, eng, 0, idx, val)
    _batch(pkg, oracle, s, eng)
    words = 4 * (eng.info()["grid"] + 1) * 72
    buf = np.zeros(words + 64, dtype=np.uint64)
    got = C.c_uint64()
    pkg._lib.check(pkg._lib.lib().tkspmv_debug_trace(eng._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size, C.byref(got)))
    assert int(got.value) == words and not buf[words:].any()
    eng.close()
    monkeypatch.delenv("TKSPMV_TRACE")
    if local == 0:
        print(f"[{name}] traced; the device-wide exchange keeps no timetable: that leg is left out")
        return
    eng = _engine(pkg, s, k, **kw)
    period = eng.debug_counters()["pace_period_ns"]
    if period == 0:
        dxs = torch.from_numpy(s.xs).cuda()
        torch.cuda.synchronize()
        eng.time_queries(dxs.data_ptr(), 16, 32)
        period = int(min(eng.time_queries(dxs.data_ptr(), 16, 32) for _ in range(3)))
    eng.close()
    assert 1000 < period < 1000000, period
    monkeypatch.setenv("TKSPMV_PACE_PERIOD", str(period))
    monkeypatch.setenv("TKSPMV_PACE", "1")
    eng = _engine(pkg, s, k, **kw)
    c = eng.debug_counters()
    assert (eng.info()["batch_mode"] >> 8) & 0xFF == local and eng.info()["batch_mode"] & 0xFF, eng.info()
    assert c["pace_period_ns"] == period and c["pace_quantum"] == 1 and c["pace_levels"] >= 1 and c["pace_tuned_us"] == 0, c
    for _ in range(3):
        _batch(pkg, oracle, s, eng)
    c = eng.debug_counters()
    assert c["batch_launches"] == 3, c
    print(f"[{name}] traced; local mode {local} on a timetable of {period} ns per query with pauses by rank {c['pace_quantum']}x{c['pace_levels']} "
          f"(the period's adaptation armed): {_some(c)}")
    eng.close()
    monkeypatch.delenv("TKSPMV_PACE_PERIOD")
    monkeypatch.delenv("TKSPMV_PACE")


def test_four_wave_workgroups_on_a_grid_too_large_to_defer(pkg, oracle, shape):
    """threads_per_wg=256: twice the default's workgroups -- more than one workgroup of block + 64 threads can select: no deferred
    selection, no fused tail, no batch kernel; stream_kernel with 4 streaming waves and select_kernel behind it."""
    eng = _engine(pkg, shape, 100, threads_per_wg=256)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 256 and g["waves"] == 4
    assert not g["defer"] and not g["batch"], f"grid {info['grid']} x block 256 was expected above block + 64 workgroups, without the batch kernel: {info}"
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    assert served == "stream" and c["batch_launches"] == 0, c
    _report("threads_per_wg=256", info, served, c)
    eng.close()


def test_one_streaming_wave_per_workgroup(pkg, oracle, shape):
    """threads_per_wg=64, waves_per_cu=4: one streaming wave (and the server wave) per workgroup, through stream_kernel. The grid is
    num_cus * 4 workgroups: above block + 64 = 128 on any device of more than 32 CUs, so the batch kernel does not run with one
    streaming wave here (nor with any other waves_per_cu: the module's note) -- asserted, so that a device or a gate that changes
    this fails the case and gets the batch checks written for it."""
    eng = _engine(pkg, shape, 100, threads_per_wg=64, waves_per_cu=4)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 64 and g["waves"] == 1 and info["n_wave_partitions"] <= info["grid"], info
    assert not g["defer"] and not g["batch"], f"a grid of {info['grid']} 64-thread workgroups was not expected to run the batch kernel: {info}"
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    assert served == "stream" and c["batch_launches"] == 0, c
    _report("threads_per_wg=64, waves_per_cu=4", info, served, c)
    eng.close()


def test_batch_kernel_with_six_streaming_waves(pkg, oracle, monkeypatch, shape):
    """threads_per_wg=384, waves_per_cu=9: few enough workgroups for the deferred selection, so the batch kernel runs with 6
    streaming waves and its server wave; single_kernel is built for 512 threads and stays out."""
    kw = dict(threads_per_wg=384, waves_per_cu=9)
    eng = _engine(pkg, shape, 100, **kw)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 384 and g["waves"] == 6
    assert g["defer"] and g["batch"], f"grid {info['grid']} x block 384 was expected to run the batch kernel: {info}"
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    assert served == "stream" and c["single_launches"] == 0 and c["batch_launches"] > 0, c
    _report(f"threads_per_wg=384, waves_per_cu=9 (local thresholds: mode {g['local']})", info, served, c)
    eng.close()
    _trace_and_timetable(pkg, oracle, monkeypatch, shape, 100, kw, "threads_per_wg=384, waves_per_cu=9")


@pytest.mark.parametrize("local", ["0", "1", "2"])
def test_batch_kernel_with_four_streaming_waves(pkg, oracle, monkeypatch, shape, local):
    monkeypatch.setenv("TKSPMV_LOCAL", local)
    kw = dict(threads_per_wg=256, waves_per_cu=4)
    eng = _engine(pkg, shape, 100, **kw)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 256 and g["waves"] == 4
    assert g["defer"] and g["batch"], f"grid {info['grid']} x block 256 was expected to run the batch kernel: {info}"
    assert g["local"] == int(local), info
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    assert served == "stream" and c["single_launches"] == 0 and c["batch_launches"] > 0, c
    if local == "0":
        assert c["checks_failed"] == 0, c
    _report(f"threads_per_wg=256, waves_per_cu=4, LOCAL={local}", info, served, c)
    eng.close()
    _trace_and_timetable(pkg, oracle, monkeypatch, shape, 100, kw, f"threads_per_wg=256, waves_per_cu=4, LOCAL={local}")


def test_more_than_512_workgroups_switch_local_thresholds_off(pkg, oracle, monkeypatch, shape):
    """waves_per_cu=32: select_local holds 512 records, so beyond 512 workgroups there are no local thresholds and no single_kernel,
    whatever TKSPMV_LOCAL says; the grid is also too large to defer."""
    monkeypatch.setenv("TKSPMV_LOCAL", "1")
    eng = _engine(pkg, shape, 100, waves_per_cu=32)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 512 and info["grid"] > 512, f"waves_per_cu=32 was expected to give more than 512 workgroups: {info}"
    assert g["local"] == 0 and not g["defer"] and not g["batch"], info
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    assert served == "stream" and c["single_launches"] == 0 and c["checks_failed"] == 0, c
    _report("waves_per_cu=32, LOCAL=1", info, served, c)
    eng.close()


def test_grid_at_the_small_matrix_boundary(pkg, oracle, shape):
    """waves_per_cu=2: the smallest grid that still gets a small matrix's settings (grid >= 64: four selector workgroups)."""
    eng = _engine(pkg, shape, 100, waves_per_cu=2)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 512 and 64 <= info["grid"] < 128, f"waves_per_cu=2 was expected to give a grid at the boundary of 64 workgroups: {info}"
    assert g["defer"] and g["selectors"] == 4, info
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    _report(f"waves_per_cu=2 (local thresholds: mode {g['local']})", info, served, c)
    eng.close()


@pytest.mark.parametrize("k", [50, 100])
def test_grid_below_64_workgroups(pkg, oracle, shape, k):
    """waves_per_cu=1: below 64 workgroups one selector, and the waves of a workgroup split into several publishing groups; with
    k = 50 the exchange serves, with k = 100 -- above 3/8 of the publishing groups -- the scores + radix-select path should. That the
    radix path ran is INFERRED: info() has no word for it; what is observed is that neither the batch kernel nor single_kernel
    exists or launches on this engine although the grid could defer (which leaves radix as choose_path's only reason), and that
    every list is exact."""
    eng = _engine(pkg, shape, k, waves_per_cu=1)
    info, g = eng.info(), _gates(eng.info())
    assert info["block"] == 512 and info["grid"] < 64, f"waves_per_cu=1 was expected to give fewer than 64 workgroups: {info}"
    if k == 50:
        assert info["n_groups"] > info["grid"] and not _radix(eng), f"several groups per workgroup and the exchange were expected: {info}"
        assert g["batch"] and g["selectors"] == 1, info
    else:
        assert _radix(eng) and not g["batch"], f"k = 100 was expected above 3/8 of the {info['n_groups']} publishing groups: {info}"
    served, c = _every_entry_point(pkg, oracle, shape, eng)
    if k == 100:
        assert c["batch_launches"] == 0 and c["single_launches"] == 0, c  # (observed; "radix" in the report is the inference)
    _report(f"waves_per_cu=1, k={k}", info, served, c)
    eng.close()


def test_invalid_geometries_are_refused(pkg):
    """threads_per_wg must be a multiple of 64 in [64, 512] (0: the default, 512) and the grid at most 1024 workgroups: anything
    else is TKSPMV_ERR_INVALID (the geometry is checked against the device, so these cases need one)."""
    m = pkg.generate_matrix(2000, 512, 12, "uniform", 3)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=10, device=0, threads_per_wg=0, waves_per_cu=0)
    info = eng.info()
    eng.close()
    assert info["block"] == 512 and info["grid"] == max(1, info["num_cus"] * 16 // 8)
    too_many = 1024 * 8 // info["num_cus"] + 1  # waves per CU that make more than 1024 workgroups of 8 waves
    for kw in (dict(threads_per_wg=32), dict(threads_per_wg=576), dict(threads_per_wg=100), dict(waves_per_cu=too_many),
               dict(threads_per_wg=64, waves_per_cu=too_many)):
        with pytest.raises(pkg.TkspmvError) as e:
            pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=10, device=0, **kw)
        assert e.value.status == pkg._lib.ERR_INVALID, kw
