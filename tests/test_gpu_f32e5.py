"""The batch kernel's compact stream (csrc/wbscsr.hpp F32E5; option F32_COMPACT, default 1): where every fp32 value of the matrix
shares its top four bits, tkspmv_create re-encodes the resident 12-bit-column stream at 5 bytes per entry (1280-byte packets instead
of 1408) and the batch kernel streams those copies -- the same entries in the same order through the same arithmetic. Each case
builds two engines on one matrix, F32_COMPACT 1 and 0, runs the same queries through enqueue_many, time_queries and enqueue_batch
and requires identical row ids, identical score bits, identical counters of failed checks, and equality with the order-matched
oracle on the canonical packing (Packed.raw(): the compact engine sums in that order too)."""
import numpy as np
import pytest

from test_gpu_single import _packed_raw

pytestmark = pytest.mark.gpu


def _pair(pkg, m, k=100, **kw):
    """(compact, plain): two engines on one matrix, F32_COMPACT 1 and 0."""
    out = []
    try:
        for v in ("1", "0"):
            pkg.set_option("F32_COMPACT", v)
            out.append(pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, **kw))
    finally:
        pkg.set_option("F32_COMPACT", None)
    return out


def _oracle_list(oracle, raw, C, m, x, k):
    yp, present = oracle.packed_scores(raw, x, m.rows, C)
    return oracle.select_topk(yp, present, k, 0.0)


def _same_as_oracle(oracle, raw, C, m, x, k, idx, val):
    ei, ev = _oracle_list(oracle, raw, C, m, x, k)
    assert np.array_equal(np.asarray(idx).astype(np.uint32), ei), "index list differs from the order-matched oracle"
    assert np.array_equal(np.ascontiguousarray(val).view(np.uint32), ev.view(np.uint32)), "scores are not bit-identical to the oracle's"


def _compare(pkg, oracle, m, xs, engines, k=100, oracle_every=1, compact=True):
    """The same queries through both engines, three ways; what the engines' info must say; identical counters of failed checks."""
    import torch
    e1, e0 = engines
    i1, i0 = e1.info(), e0.info()
    assert i0["batch_compact"] == 0 and i0["batch_packet_bytes"] == 1408 and i0["batch_stream_bytes"] == i0["n_packets"] * 1408
    assert i1["batch_compact"] == (1 if compact else 0) and i1["batch_packet_bytes"] == (1280 if compact else 1408)
    assert i1["batch_stream_bytes"] == i1["n_packets"] * i1["batch_packet_bytes"]
    for key in ("packed_bytes", "n_packets", "packet_entries", "n_wave_partitions", "batch_mode"):
        assert i1[key] == i0[key], key
    _, raw, C = _packed_raw(pkg, m, e1, k)
    assert raw[1] == 1408  # (the canonical packing: what the oracle reads)
    n = xs.shape[0]
    dxs = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    torch.cuda.synchronize()
    # enqueue_many into the engine's own pair: the last query wins
    got = []
    for e in (e1, e0):
        e.enqueue_many(dxs.data_ptr(), n, n)
        got.append(e.read_result())
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    _same_as_oracle(oracle, raw, C, m, xs[n - 1], k, got[0][1], got[0][0])
    # time_queries (the benchmark's entry point), n + 3 queries cycling over the n vectors
    got = []
    for e in (e1, e0):
        assert e.time_queries(dxs.data_ptr(), n, n + 3) > 0
        got.append(e.read_result())
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    _same_as_oracle(oracle, raw, C, m, xs[(n + 2) % n], k, got[0][1], got[0][0])
    # enqueue_batch into caller buffers: every list
    res = []
    for e in (e1, e0):
        oi = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
        ov = torch.full((n, k), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.enqueue_batch(dxs.data_ptr(), n, oi.data_ptr(), ov.data_ptr())
        e.synchronize()
        res.append((oi.cpu().numpy(), ov.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))
    for q in range(0, n, oracle_every):
        _same_as_oracle(oracle, raw, C, m, xs[q], k, res[0][0][q], res[0][1][q])
    c1, c0 = e1.debug_counters(), e0.debug_counters()
    assert c1["checks_failed"] == c0["checks_failed"], (c1, c0)
    return c1


def _queries(pkg, cols, n, seed):
    return np.stack([pkg.create_sample_vector(cols, True, False, True, seed + i) for i in range(n)])


def _close(engines):
    for e in engines:
        e.close()


@pytest.fixture(scope="module")
def m125(pkg):
    return pkg.generate_matrix(125000, 1024, 20, "gamma", 2)


@pytest.fixture(scope="module")
def m20(pkg):
    return pkg.generate_matrix(20000, 1024, 20, "gamma", 3)


def test_narrow_matrix_with_one_or_two_packets_per_partition(pkg, oracle):
    m = pkg.generate_matrix(5000, 300, 12, "gamma", 4)
    engines = _pair(pkg, m, k=50)
    _compare(pkg, oracle, m, _queries(pkg, 300, 9, 100), engines, k=50)
    _close(engines)


def test_two_launches_over_three_rotating_stream_copies(pkg, oracle, m125):
    engines = _pair(pkg, m125, stream_replicas=3)
    _compare(pkg, oracle, m125, _queries(pkg, 1024, 33, 200), engines)
    _close(engines)


def test_local_thresholds_with_pacing_measured_at_create(pkg, oracle):
    m = pkg.generate_matrix(400000, 1024, 20, "gamma", 6)
    engines = _pair(pkg, m)
    assert (engines[0].info()["batch_mode"] >> 8) & 0xFF, "this size is expected to stream with workgroup-local thresholds"
    # (the order-matched oracle takes 0.2 s per query at this size: every fifth list against it, all forty against the other engine)
    c = _compare(pkg, oracle, m, _queries(pkg, 1024, 40, 300), engines, oracle_every=5)
    assert c["pace_tuned_us"] > 0, c
    _close(engines)


def test_placeholders_of_empty_rows_under_negative_scores(pkg, oracle, m125):
    """Every 7th row emptied (a SKIP entry each: +0.0, which no compact word says) and negated queries: every real score is negative,
    the placeholders' products are signed zeros, the thresholds start at min_score 0."""
    keep = (m125.row % 7) != 0
    m = pkg.CooMatrix(m125.rows, m125.cols, m125.row[keep], m125.col[keep], m125.val[keep])
    xs = _queries(pkg, 1024, 12, 400)
    xs[::2] *= np.float32(-1.0)
    engines = _pair(pkg, m)
    _compare(pkg, oracle, m, xs, engines)
    _close(engines)


def test_the_last_two_columns(pkg, oracle, m20):
    col = m20.col.copy()
    col[::3] = 1023
    col[1::3] = 1022
    order = np.lexsort((col, m20.row))
    m = pkg.CooMatrix(m20.rows, m20.cols, m20.row[order], col[order], m20.val[order])
    engines = _pair(pkg, m)
    _compare(pkg, oracle, m, _queries(pkg, 1024, 8, 500), engines)
    _close(engines)


@pytest.mark.parametrize("repair", ["host", "stream"])
def test_the_exact_kernel_repairs_from_the_compact_copy(pkg, oracle, monkeypatch, m125, repair):
    """SIGNATURES=0 and queries that change direction: thresholds carried from +x fail the check of -x, and the exact kernel answers
    the flagged queries again -- in the stream (REPAIR=stream) or when the host waits (REPAIR=host) -- from the compact copies."""
    monkeypatch.setenv("TKSPMV_SIGNATURES", "0")
    monkeypatch.setenv("TKSPMV_REPAIR", repair)
    xs = _queries(pkg, 1024, 40, 600)
    xs[[9, 21, 22, 35]] *= np.float32(-1.0)
    engines = _pair(pkg, m125)
    assert (engines[0].info()["batch_mode"] >> 8) & 0xFF
    c = _compare(pkg, oracle, m125, xs, engines)
    assert c["checks_failed"] > 0, c
    _close(engines)


@pytest.mark.parametrize("what", ["negative", "zero", "wide"])
def test_matrices_the_predicate_refuses_run_as_before(pkg, oracle, m20, what):
    val = m20.val.copy()
    val[12345] = {"negative": -0.25, "zero": 0.0, "wide": 2.0 ** -40}[what]
    m = pkg.CooMatrix(m20.rows, m20.cols, m20.row, m20.col, val)
    engines = _pair(pkg, m)
    _compare(pkg, oracle, m, _queries(pkg, 1024, 6, 700), engines, compact=False)
    _close(engines)


@pytest.mark.parametrize("what", ["scaled", "negated"])
def test_other_windows_of_32_binades(pkg, oracle, m20, what):
    val = (m20.val * np.float32(2.0 ** 30 if what == "scaled" else -1.0)).astype(np.float32)
    m = pkg.CooMatrix(m20.rows, m20.cols, m20.row, m20.col, val)
    engines = _pair(pkg, m)
    _compare(pkg, oracle, m, _queries(pkg, 1024, 6, 800), engines)
    _close(engines)


def test_an_engine_created_from_a_packed_file(pkg, oracle, m20, tmp_path):
    import torch
    k = 100
    src = pkg.SpMV(m20.row, m20.col, m20.val, m20.rows, m20.cols, k=k, device=0)
    packed, raw, C = _packed_raw(pkg, m20, src, k)
    path = str(tmp_path / "m.tkspmv")
    packed.save(path)
    eng = pkg.SpMV.from_packed(pkg.Packed.load(path), k=k, device=0)
    assert src.info()["batch_compact"] == 1 and eng.info()["batch_compact"] == 1 and eng.info()["batch_packet_bytes"] == 1280
    xs = _queries(pkg, 1024, 7, 900)
    dxs = torch.from_numpy(xs).cuda()
    res = []
    for e in (eng, src):
        oi = torch.full((7, k), -1, dtype=torch.int32, device="cuda")
        ov = torch.full((7, k), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.enqueue_batch(dxs.data_ptr(), 7, oi.data_ptr(), ov.data_ptr())
        e.synchronize()
        res.append((oi.cpu().numpy(), ov.cpu().numpy()))
        e.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))
    for q in range(7):
        _same_as_oracle(oracle, raw, C, m20, xs[q], k, res[0][0][q], res[0][1][q])


def test_the_read_probe_reads_the_compact_copies(pkg):
    """tkspmv_time_stream_read must read what the batch kernel reads -- the 1280-byte packets, with the 20-bytes-per-lane probe --: a
    pass of the load-only probe is then shorter than a query, and shorter than the same pass on an engine that streams the canonical
    1408-byte packets (F32_COMPACT=0; 9.1 % more bytes: at least 3 % more time is asked)."""
    import torch
    m = pkg.generate_matrix(400000, 1024, 20, "gamma", 6)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, stream_replicas=8)
    assert eng.info()["batch_compact"] == 1
    xs = _queries(pkg, 1024, 32, 1000)
    dxs = torch.from_numpy(xs).cuda()
    torch.cuda.synchronize()
    eng.time_queries(dxs.data_ptr(), 32, 256)  # (clocks)
    query_ns = min(eng.time_queries(dxs.data_ptr(), 32, 512) for _ in range(3))
    read_ns = min(eng.time_stream_read(64) for _ in range(3))
    print(f"\n[400k rows, 8 copies] load-only pass {read_ns / 1e3:.2f} us, query {query_ns / 1e3:.2f} us")
    assert 0 < read_ns < query_ns
    # the probe of an engine on the canonical stream moves 1408 / 1280 = 1.10 x the bytes: medians of five passes each, and a
    # margin of two thirds of the difference for what boxes vary between runs (+-1.6 % in the records)
    med = sorted(eng.time_stream_read(64) for _ in range(5))[2]
    eng.close()
    pkg.set_option("F32_COMPACT", "0")
    try:
        plain = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, stream_replicas=8)
    finally:
        pkg.set_option("F32_COMPACT", None)
    assert plain.info()["batch_compact"] == 0
    plain.time_stream_read(64)
    med_plain = sorted(plain.time_stream_read(64) for _ in range(5))[2]
    plain.close()
    print(f"[400k rows, 8 copies] median load-only pass {med / 1e3:.2f} us over 1280-byte packets, {med_plain / 1e3:.2f} us over 1408-byte packets")
    assert med < 0.97 * med_plain
