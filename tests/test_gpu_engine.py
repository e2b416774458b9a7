"""GPU tests of the engine boundary beyond plain parity: the reference's golden vectors through the HIP path, edge
cases (empty rows, k > rows, single row, rows longer than a packet, k = 1024, wide x), size-independent properties at
the full BASELINE size, the drop-in executable's CSV, and the asynchronous/device-pointer entry points.
(_expected() is the bit-exact leg: it re-packs with the product's own host packer and the engine's partition hint, so it shares
the packer with the product; the gold comparisons in the same tests are the independent leg -- see test_gpu_parity.py.)"""
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASE_FILES = sorted(p for p in glob.glob(os.path.join(GOLD, "gold_*.npz")) if re.search(r"_\d+x\d+\.npz$", p))
RTOL = 1e-4


def _expected(pkg, oracle, m, x, k, eng, min_score=0.0, first_row=0):
    info = eng.info()
    C = info["packet_entries"] // 64
    packed = pkg.Packed(m, k=k, nnz_per_lane=C, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    yp, present = oracle.packed_scores(packed.raw(), x, m.rows, C)
    return oracle.select_topk(yp, present, k, min_score, first_row)


@pytest.mark.parametrize("path", CASE_FILES, ids=[os.path.basename(p) for p in CASE_FILES])
def test_reference_golden_vectors_through_the_gpu(pkg, oracle, path):
    z = np.load(path)
    cases = json.loads(bytes(z["cases"]).decode())
    m = pkg.CooMatrix(int(z["rows"]), int(z["cols"]), z["row"], z["col"], z["val"])
    for c in cases:
        t, k = c["tag"], c["k"]
        x = z[f"x_{t}"]
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=k, device=0)
        eng()
        val, idx = eng.read_result()
        ei, ev = _expected(pkg, oracle, m, x, k, eng)
        assert np.array_equal(idx, ei) and np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        gi, gv = z[f"idx_{t}"], z[f"val_{t}"]
        if np.all(gv > 0) and len(np.unique(gv)) == k:  # full list of distinct positive scores: the north-star bar
            assert set(idx.tolist()) == set(gi.tolist())
            assert np.allclose(val, gv, rtol=RTOL, atol=0)
        else:  # fillers / zero scores: same positive part, (0, 0.0) padding behind it
            npos = int((gv > 0).sum())
            assert set(idx[:npos].tolist()) == set(gi[:npos].tolist())
            assert np.allclose(val[:npos], gv[:npos], rtol=RTOL, atol=0)
            assert np.all(val[npos:] == 0)
        eng.close()


def test_reference_golden_vectors_through_the_multi_query_path(pkg, oracle):
    """The same golden vectors through tkspmv_enqueue_multi: every case's queries share passes (different x per query)."""
    import torch
    for path in CASE_FILES:
        z = np.load(path)
        cases = json.loads(bytes(z["cases"]).decode())
        m = pkg.CooMatrix(int(z["rows"]), int(z["cols"]), z["row"], z["col"], z["val"])
        if m.cols > 1024:
            continue
        by_k = {}
        for c in cases:
            by_k.setdefault(c["k"], []).append(c["tag"])
        for k, tags in by_k.items():
            eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, multi_q=2)
            if eng.info()["multi_q"] == 0:  # k above the publishing groups: no multi-query kernel for this engine
                eng.close()
                continue
            xs = np.stack([z[f"x_{t}"] for t in tags]).astype(np.float32)
            dxs = torch.from_numpy(xs).cuda()
            out_i = torch.zeros((len(tags), k), dtype=torch.int32, device="cuda")
            out_v = torch.zeros((len(tags), k), dtype=torch.float32, device="cuda")
            eng.enqueue_multi(dxs.data_ptr(), len(tags), out_i.data_ptr(), out_v.data_ptr())
            eng.synchronize()
            for j, t in enumerate(tags):
                idx, val = out_i[j].cpu().numpy().view(np.uint32), out_v[j].cpu().numpy()
                gi, gv = z[f"idx_{t}"], z[f"val_{t}"]
                npos = k if (np.all(gv > 0) and len(np.unique(gv)) == k) else int((gv > 0).sum())
                assert set(idx[:npos].tolist()) == set(gi[:npos].tolist()), (os.path.basename(path), t)
                assert np.allclose(val[:npos], gv[:npos], rtol=RTOL, atol=0)
                assert np.all(val[npos:] <= 0)
            eng.close()


def _coo(pkg, rows, cols, lens, seed=0, neg=False):
    rng = np.random.RandomState(seed)
    r, c, v = [], [], []
    for i, n in enumerate(lens):
        cs = np.sort(rng.randint(0, cols, n))
        vs = rng.rand(n).astype(np.float32) - (0.5 if neg else 0.0)
        r += [i] * n
        c += cs.tolist()
        v += vs.tolist()
    return pkg.CooMatrix(rows, cols, np.array(r, np.uint32), np.array(c, np.uint32), np.array(v, np.float32))


@pytest.mark.parametrize("name,lens,cols,k", [
    ("empty_rows", [3, 0, 0, 5, 1, 0, 7, 2, 0, 0, 0, 4] * 40, 64, 20),
    ("single_row", [9], 32, 4),
    ("single_entry", [1], 8, 1),
    ("k_gt_rows", [2, 3, 4], 16, 50),
    ("long_rows", [1100, 1, 300, 2, 257, 256, 255, 1, 1, 700], 1024, 5),
    ("one_nnz_rows", [1] * 3000, 128, 100),
    ("k_1024", [6] * 5000, 256, 1024),
    ("wide_x", [30] * 2000, 16384, 64),
    ("trailing_empty", [4, 4, 4, 0, 0, 0], 16, 3),
])
def test_edge_cases(pkg, oracle, name, lens, cols, k):
    m = _coo(pkg, len(lens) + (3 if name == "trailing_empty" else 0), cols, lens, seed=len(lens))
    x = pkg.create_sample_vector(cols, True, False, True, 77)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=k, device=0)
    eng()
    val, idx = eng.read_result()
    ei, ev = _expected(pkg, oracle, m, x, k, eng)
    assert np.array_equal(idx, ei), name
    assert np.array_equal(val.view(np.uint32), ev.view(np.uint32)), name
    # against the gold: the rows with a positive score agree (set), scores within tolerance
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, x, k)
    npos = int((gv > 0).sum())
    assert set(idx[:npos].tolist()) == set(gi[:npos].tolist())
    assert np.allclose(val[:npos], gv[:npos], rtol=RTOL, atol=0)
    y = eng.scores()
    ys, present = oracle.scores_f32_seq(m.row, m.col, m.val, x, m.rows)
    assert np.allclose(y[present.astype(bool)], ys[present.astype(bool)], rtol=RTOL, atol=1e-30)
    assert np.all(y[~present.astype(bool)] == 0)
    eng.close()


def test_negative_scores_and_min_score(pkg, oracle):
    """General (signed) matrices: rows scoring below min_score never come back (gold: initial worst = 0)."""
    m = _coo(pkg, 4000, 128, [8] * 4000, seed=3, neg=True)
    x = pkg.create_sample_vector(128, True, False, True, 9)
    for min_score in (0.0, -1e30, 0.05):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=100, device=0, min_score=min_score)
        eng()
        val, idx = eng.read_result()
        ei, ev = _expected(pkg, oracle, m, x, 100, eng, min_score=min_score)
        assert np.array_equal(idx, ei) and np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        eng.close()
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, x, 100)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=100, device=0)
    eng()
    val, idx = eng.read_result()
    assert set(idx.tolist()) == set(gi.tolist()) and np.allclose(val, gv, rtol=RTOL, atol=0)
    eng.close()


def test_ignore_matrix_values(pkg, oracle):
    m = pkg.generate_matrix(5000, 256, 10, "uniform", 12)
    x = pkg.create_sample_vector(256, True, False, True, 2)
    eng = pkg.SpMV(m.row, m.col, None, m.rows, m.cols, vec=x, k=16, device=0)  # -v: all ones
    eng()
    val, idx = eng.read_result()
    ones = np.ones_like(m.val)
    gi, gv = oracle.gold_topk(m.row, m.col, ones, x, 16)
    assert set(idx.tolist()) == set(gi.tolist()) and np.allclose(val, gv, rtol=RTOL, atol=0)
    eng.close()


@pytest.fixture(scope="module")
def big(pkg):
    m = pkg.generate_matrix(1000000, 1024, 20, "gamma", 2)  # BASELINE configs[1]
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    yield m, eng
    eng.close()


def test_full_size_parity_and_properties(pkg, oracle, big):
    m, eng = big
    x = pkg.create_sample_vector(1024, True, False, True, 4242)
    eng.reset(x)
    eng()
    val, idx = eng.read_result()
    # (1) the gold itself at full size (19.5M nnz takes the oracle well under a second)
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, x, 100)
    y64, present = oracle.scores_f64(m.row, m.col, m.val, x, m.rows)
    if set(idx.tolist()) != set(gi.tolist()):
        kth = np.sort(y64)[-100]
        for r in set(idx.tolist()) ^ set(gi.tolist()):
            assert abs(y64[r] - kth) <= 2e-6 * kth, "only k-th boundary near-ties may differ"
    assert np.allclose(np.sort(val), np.sort(gv), rtol=RTOL, atol=0)
    # (2) sortedness + uniqueness + every returned score is that row's score
    assert np.all(val[:-1] >= val[1:]) and len(set(idx.tolist())) == 100
    assert np.allclose(val, y64[idx], rtol=RTOL, atol=0)
    # (3) nothing outside the list beats the list (checksum of the whole score vector through the SpMV-only kernel)
    y = eng.scores()
    assert np.allclose(y, y64, rtol=RTOL, atol=1e-12)
    rest = np.ones(m.rows, dtype=bool)
    rest[idx] = False
    assert y[rest].max() <= val[-1]
    # (4) idempotence and scale equivariance: same x twice -> identical bits; 2x -> same rows, doubled scores
    eng()
    val2, idx2 = eng.read_result()
    assert np.array_equal(idx, idx2) and np.array_equal(val.view(np.uint32), val2.view(np.uint32))
    eng.reset(2.0 * x)
    eng()
    val3, idx3 = eng.read_result()
    assert np.array_equal(idx3, idx) and np.array_equal(val3, 2.0 * val)
    # (5) bit-exact against the order-matched oracle at full size
    ei, ev = _expected(pkg, oracle, m, x, 100, eng)
    assert np.array_equal(idx, ei) and np.array_equal(val.view(np.uint32), ev.view(np.uint32))


def test_k8_is_the_32_partition_result(pkg, oracle, big):
    """BASELINE configs[2]: 32 row partitions with K=8 lists each, query K=8. The union of the per-partition top-8
    contains the global top-8, so the partitioned model and the exact engine must agree."""
    m, _ = big
    x = pkg.create_sample_vector(1024, True, False, True, 99)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=8, device=0, partitions=32, k_per_partition=8)
    assert eng.info()["partitions"] == 32 and eng.info()["k_per_partition"] == 8
    eng()
    val, idx = eng.read_result()
    y, present = oracle.scores_f32_seq(m.row, m.col, m.val, x, m.rows)
    per = (m.rows + 31) // 32  # host_spmv_bscsr.cpp:136
    cand_i, cand_v = [], []
    for p in range(32):
        a, b = p * per, min((p + 1) * per, m.rows)
        pi, pv = oracle.select_topk(y[a:b], present[a:b], 8, 0.0, first_row=a)
        cand_i += pi.tolist()
        cand_v += pv.tolist()
    order = np.lexsort((-np.array(cand_i, np.int64), -np.array(cand_v, np.float64)))[:8]
    assert set(idx.tolist()) == set(np.array(cand_i)[order].tolist())
    assert np.allclose(val, np.array(cand_v, np.float32)[order], rtol=RTOL, atol=0)
    eng.close()


def test_device_pointers_async_and_replicas(pkg, oracle):
    import torch
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 8)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 500 + i) for i in range(5)])
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros(5, 100, dtype=torch.int32, device="cuda")
    out_v = torch.zeros(5, 100, dtype=torch.float32, device="cuda")
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, stream_replicas=3)
    stream = torch.cuda.current_stream().cuda_stream
    for q in range(5):  # caller-owned device buffers, caller's stream, no host sync in between
        eng.enqueue(dxs[q].data_ptr(), out_i[q].data_ptr(), out_v[q].data_ptr(), stream)
    torch.cuda.synchronize()
    for q in range(5):
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[q], 100)
        assert set(out_i[q].cpu().numpy().astype(np.uint32).tolist()) == set(gi.tolist())
        assert np.allclose(out_v[q].cpu().numpy(), gv, rtol=RTOL, atol=0)
    t = eng.profile(dxs.data_ptr(), 5, 20)
    assert t["stream_kernel_ns"] > 0 and t["query_ns"] > 0 and t["scores_kernel_ns"] > 0
    eng.reset_device(dxs[2].data_ptr())
    eng()
    val, idx = eng.read_result()
    assert np.array_equal(idx.astype(np.int64), out_i[2].cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
    # first_row offsets the returned ids (row-sharded use)
    eng2 = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=xs[2], k=100, device=0, first_row=123456)
    eng2()
    val2, idx2 = eng2.read_result()
    assert np.array_equal(idx2, idx + 123456) and np.array_equal(val2, val)
    eng.close()
    eng2.close()


def test_run_before_query_is_an_error(pkg):
    m = pkg.generate_matrix(100, 32, 4, "uniform", 1)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=4, device=0)
    with pytest.raises(pkg.TkspmvError) as e:
        eng()
    assert e.value.status == pkg._lib.ERR_STATE
    eng.close()


def test_drop_in_executable_csv(pkg, oracle, tmp_path):
    """The call site of test_spmv_topk.py:63,79-82: same flags, GPU-host CSV schema, zero errors against its gold."""
    exe = os.path.join(ROOT, "bin", "approximate-spmv-mi355x-topk")
    g = pkg.generate_matrix(10000, 1024, 20, "gamma", 1)  # BASELINE configs[0] shape, generator output format
    p = tmp_path / "matrix_10000_1024_20_gamma.mtx"
    pkg.write_mtx(str(p), g, index_base=1)
    # read zero-based (the reference's compiled-in behaviour, the default): the one-based file is refused with a hint
    r = subprocess.run([exe, "-t", "1", "-m", str(p), "-k", "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "TKSPMV_INDEX_BASE=1" in r.stderr
    env = dict(os.environ, TKSPMV_SEED="5", TKSPMV_INDEX_BASE="1")
    r = subprocess.run([exe, "-t", "4", "-m", str(p), "-k", "100", "-i", "0", "-r"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == ("iteration,error_idx,error_val,sw_full_time_ms,sw_topk_time_ms,hw_setup_time_ms,"
                        "hw_spmv_only_time_ms,hw_exec_time_ms,readback_time_ms,k,sw_res_idx,sw_res_val,hw_res_idx,"
                        "hw_res_val")
    assert len(lines) == 5
    for i, ln in enumerate(lines[1:]):
        f = ln.split(",")
        assert len(f) == 14 and int(f[0]) == i and int(f[9]) == 100
        sw_idx, hw_idx = f[10].split(";"), f[12].split(";")
        assert len(sw_idx) == 100 and len(hw_idx) == 100
        assert set(sw_idx) == set(hw_idx)            # same top-k index set as the CPU gold
        assert int(f[2]) == 0                        # error_val: |diff| <= 1e-5 everywhere
        assert np.allclose(np.array(f[11].split(";"), float), np.array(f[13].split(";"), float), rtol=1e-4, atol=1e-6)
    # -d prints the verbose form and still exits 0
    r = subprocess.run([exe, "-d", "-t", "1", "-m", str(p), "-k", "8"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "hw results=" in r.stdout and "precision=1" in r.stdout
    # TKSPMV_CACHE_DIR: the first run writes the packed matrix, the second reads it (no MatrixMarket parsing, no
    # packing) and must print the same results, software gold included (its COO is decoded from the packed matrix)
    cache = tmp_path / "cache"
    cache.mkdir()
    env_c = dict(env, TKSPMV_CACHE_DIR=str(cache))
    outs = []
    for run in range(2):
        r = subprocess.run([exe, "-d", "-t", "2", "-m", str(p), "-k", "100", "-r"], capture_output=True, text=True,
                           env=env_c, timeout=300)
        assert r.returncode == 0, r.stderr
        assert ("packed matrix read from" in r.stdout) == (run == 1)
        outs.append([ln for ln in r.stdout.split("\n") if ") document " in ln])
    assert len(list(cache.glob("*.tkspmv"))) == 1
    assert outs[0] == outs[1] and len(outs[0]) >= 400  # sw + hw lists of both iterations
    # -a: the comparator's half-precision mode -> fp16 values; the CSV reports its precision against the fp32 gold
    r = subprocess.run([exe, "-t", "3", "-m", str(p), "-k", "100", "-r", "-a"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    for ln in r.stdout.strip().split("\n")[1:]:
        f = ln.split(",")
        sw_idx, hw_idx = f[10].split(";"), f[12].split(";")
        assert len(set(sw_idx) & set(hw_idx)) >= 90
        assert np.allclose(np.array(f[11].split(";"), float), np.array(f[13].split(";"), float), rtol=5e-3, atol=1e-6)
    # TKSPMV_FIXED_WIDTH: the FPGA builds' fixed-point arithmetic (the reference's compile-time FIXED_WIDTH)
    r = subprocess.run([exe, "-t", "3", "-m", str(p), "-k", "100", "-r"], capture_output=True, text=True,
                       env=dict(env, TKSPMV_FIXED_WIDTH="20"), timeout=300)
    assert r.returncode == 0, r.stderr
    for ln in r.stdout.strip().split("\n")[1:]:
        f = ln.split(",")
        sw_idx, hw_idx = f[10].split(";"), f[12].split(";")
        assert len(set(sw_idx) & set(hw_idx)) >= 95
        assert np.allclose(np.array(f[11].split(";"), float), np.array(f[13].split(";"), float), rtol=2e-3, atol=1e-6)
    r = subprocess.run([exe, "-t", "1", "-m", str(p)], capture_output=True, text=True, env=dict(env, TKSPMV_FIXED_WIDTH="40"),
                       timeout=300)
    assert r.returncode == 1 and "TKSPMV_FIXED_WIDTH" in r.stderr


def test_executable_generates_its_matrix_in_memory():
    """TKSPMV_GENERATE=rows,cols,nnz,dist,seed: the drop-in executable without a MatrixMarket file (the reference's grid reaches 7 GB
    of text per matrix). 2M rows x 20 = 40M non-zeros: the size from which the per-iteration software gold forms its row sums with
    several threads -- every iteration's list must equal that gold's, index for index."""
    exe = os.path.join(ROOT, "bin", "approximate-spmv-mi355x-topk")
    env = dict(os.environ, TKSPMV_GENERATE="2000000,1024,20,gamma,3", TKSPMV_SEED="5")
    r = subprocess.run([exe, "-t", "3", "-k", "100", "-r"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    lines = [ln.split(",") for ln in r.stdout.strip().split("\n") if ln and ln[0].isdigit()]
    assert len(lines) == 3 and all(int(f[1]) == 0 for f in lines), r.stdout[:600]
    r = subprocess.run([exe, "-t", "1", "-k", "100"], capture_output=True, text=True, env=dict(env, TKSPMV_GENERATE="12,x"), timeout=60)
    assert r.returncode == 1 and "TKSPMV_GENERATE" in r.stderr


def test_reference_side_host_program(pkg):
    """oracle/_ref/host_spmv_topk_mi355x (built in the build container from oracle/ref_host_mi355x.cpp against the
    reference's OWN headers: its Options, readMtx, coo_t, create_sample_vector, gold and checks around this engine's C ABI,
    INTEGRATION.md section 2) runs the reference's flow end to end: every iteration's list equals the reference gold's."""
    exe = os.path.join(ROOT, "oracle", "_ref", "host_spmv_topk_mi355x")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref was not built (no reference tree at build time)")
    for impl in ("0", "1", "2"):
        r = subprocess.run([exe, "-m", os.path.join(GOLD, "small_0indexed.mtx"), "-k", "20", "-t", "4", "-i", impl],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (impl, r.stdout[-500:], r.stderr[-500:])
        lines = [ln.split(",") for ln in r.stdout.strip().split("\n") if ln and ln[0].isdigit()]
        assert len(lines) == 4 and all(float(f[4]) == 1.0 and int(f[2]) == 0 for f in lines), (impl, r.stdout)


# ---- BASELINE configs[4]: Q1.7 fixed-point values ("FIXED_WIDTH-style" reduced precision) ----------------------------
@pytest.mark.parametrize("rows,cols,nnz,k,seed", [(3000, 512, 40, 100, 1), (60000, 512, 40, 100, 2),
                                                  (20000, 1024, 20, 8, 3), (5000, 3000, 30, 50, 4), (5000, 6000, 30, 50, 5)])
def test_q1_7_bit_exact_against_integer_model(pkg, oracle, rows, cols, nnz, k, seed):
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", seed)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, precision=pkg.Q1_7)
    assert eng.info()["precision"] == pkg.Q1_7 and eng.info()["packed_bytes"] < 3.2 * m.nnz + 64 * rows
    for q in range(2):
        x = pkg.create_sample_vector(cols, True, False, True, 10 * seed + q + 1)
        eng.reset(x)
        eng()
        val, idx = eng.read_result()
        y, present = oracle.q17_scores(m.row, m.col, m.val, x, m.rows)
        ei, ev = oracle.select_topk(y, present, k)
        assert np.array_equal(idx, ei), "index list differs from the integer model"
        assert np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        ys = eng.scores()
        assert np.array_equal(ys.view(np.uint32), y.view(np.uint32))  # every row, bit for bit
    eng.close()


def test_q1_7_wraps_and_saturates_like_the_model(pkg, oracle):
    """Values above 1.0, long rows and a large x: products wrap at 2.0, sums wrap at 2.0, conversion saturates."""
    rng = np.random.RandomState(0)
    lens = [300, 5, 1, 64, 257, 2, 900] * 20
    r, c, v = [], [], []
    for i, n in enumerate(lens):
        r += [i] * n
        c += np.sort(rng.randint(0, 64, n)).tolist()
        v += (rng.rand(n) * 2.5).astype(np.float32).tolist()  # some above the Q1.7 range
    m = pkg.CooMatrix(len(lens), 64, np.array(r, np.uint32), np.array(c, np.uint32), np.array(v, np.float32))
    x = (rng.rand(64) * 1.9).astype(np.float32)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=16, device=0, precision=pkg.Q1_7)
    eng()
    val, idx = eng.read_result()
    y, present = oracle.q17_scores(m.row, m.col, m.val, x, m.rows)
    ei, ev = oracle.select_topk(y, present, 16)
    assert np.array_equal(idx, ei) and np.array_equal(val, ev)
    assert np.array_equal(eng.scores(), y)
    eng.close()


def test_q1_7_full_size_config(pkg, oracle):
    """BASELINE configs[4]: 1M x 512, 40 nnz/row, K=100. Bit-exact against the integer model; precision@100 against
    the fp32 gold is REPORTED (8-bit scores of ~20-term dot products are very coarse), not asserted beyond sanity."""
    m = pkg.generate_matrix(1000000, 512, 40, "gamma", 5)
    x = pkg.create_sample_vector(512, True, False, True, 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=100, device=0, precision=pkg.Q1_7)
    eng()
    val, idx = eng.read_result()
    y, present = oracle.q17_scores(m.row, m.col, m.val, x, m.rows)
    ei, ev = oracle.select_topk(y, present, 100)
    assert np.array_equal(idx, ei) and np.array_equal(val, ev)
    gi, _ = oracle.gold_topk(m.row, m.col, m.val, x, 100)
    precision = len(set(idx.tolist()) & set(gi.tolist())) / 100.0
    print(f"Q1.7 precision@100 vs fp32 gold: {precision:.2f}")
    assert 0.0 <= precision <= 1.0
    eng.close()


# ---- TKSPMV_FIXED: the FPGA's real_type for any FIXED_WIDTH (reference builds: 20/21/25/26/32 bits) --------------------
@pytest.mark.parametrize("width", [8, 20, 21, 25, 26, 32])
@pytest.mark.parametrize("rows,cols,nnz,k,seed", [(3000, 512, 40, 100, 1), (60000, 1024, 20, 100, 2), (5000, 3000, 30, 50, 4),
                                                  (5000, 6000, 30, 50, 5)])
def test_fixed_point_bit_exact_against_integer_model(pkg, oracle, width, rows, cols, nnz, k, seed):
    """Scores of every row and the top-k, bit for bit against the W-bit integer model (oracle_fixed_scores: plain
    right-aligned integers and 64-bit products; the kernel works on left-aligned Q1.31 words)."""
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", seed)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, precision=pkg.FIXED, fixed_width=width)
    assert eng.info()["precision"] == pkg.FIXED and eng.info()["fixed_width"] == width
    for q in range(2):
        x = pkg.create_sample_vector(cols, True, False, True, 10 * seed + q + 1)
        if q == 1:
            x = (x * np.float32(25.0)).astype(np.float32)  # larger scores: some sums wrap at 2.0
        eng.reset(x)
        eng()
        val, idx = eng.read_result()
        y, present = oracle.fixed_scores(m.row, m.col, m.val, x, m.rows, width)
        ei, ev = oracle.select_topk(y, present, k)
        assert np.array_equal(idx, ei), "index list differs from the integer model"
        assert np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        assert np.array_equal(eng.scores().view(np.uint32), y.view(np.uint32))  # every row
    eng.close()


def test_fixed_point_width_8_is_q1_7(pkg):
    m = pkg.generate_matrix(40000, 512, 40, "gamma", 8)
    x = (pkg.create_sample_vector(512, True, False, True, 5) * np.float32(30.0)).astype(np.float32)
    a = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=64, device=0, precision=pkg.FIXED, fixed_width=8)
    b = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=64, device=0, precision=pkg.Q1_7)
    a()
    b()
    va, ia = a.read_result()
    vb, ib = b.read_result()
    assert np.array_equal(ia, ib) and np.array_equal(va, vb)
    assert np.array_equal(a.scores(), b.scores())
    a.close()
    b.close()


def test_fixed_point_wraps_and_saturates_like_the_model(pkg, oracle):
    rng = np.random.RandomState(0)
    lens = [300, 5, 1, 64, 257, 2, 900] * 20
    r, c, v = [], [], []
    for i, n in enumerate(lens):
        r += [i] * n
        c += np.sort(rng.randint(0, 64, n)).tolist()
        v += (rng.rand(n) * 2.5).astype(np.float32).tolist()  # some above the range
    m = pkg.CooMatrix(len(lens), 64, np.array(r, np.uint32), np.array(c, np.uint32), np.array(v, np.float32))
    x = (rng.rand(64) * 1.9).astype(np.float32)
    for width in (20, 32):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=16, device=0, precision=pkg.FIXED, fixed_width=width)
        eng()
        val, idx = eng.read_result()
        y, present = oracle.fixed_scores(m.row, m.col, m.val, x, m.rows, width)
        ei, ev = oracle.select_topk(y, present, 16)
        assert np.array_equal(idx, ei) and np.array_equal(val, ev)
        assert np.array_equal(eng.scores(), y)
        eng.close()


@pytest.mark.parametrize("width,floor", [(20, 0.9), (25, 0.97), (32, 0.99)])
def test_fixed_point_full_size_precision_against_the_fp32_gold(pkg, oracle, width, floor):
    """BASELINE configs[1]'s matrix with the reference's fixed-point builds: bit-exact against the integer model, and
    precision@100 against the fp32 gold -- the reference's own acceptance metric (host_spmv_bscsr.cpp:646-650; its
    published figure: ~97-98 % at 20 bits, >= 99 % at 32)."""
    m = pkg.generate_matrix(1000000, 1024, 20, "gamma", 2)
    x = pkg.create_sample_vector(1024, True, False, True, 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=100, device=0, precision=pkg.FIXED, fixed_width=width)
    eng()
    val, idx = eng.read_result()
    y, present = oracle.fixed_scores(m.row, m.col, m.val, x, m.rows, width)
    ei, ev = oracle.select_topk(y, present, 100)
    assert np.array_equal(idx, ei) and np.array_equal(val, ev)
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, x, 100)
    precision = len(set(idx.tolist()) & set(gi.tolist())) / 100.0
    print(f"fixed point W={width}: precision@100 vs fp32 gold {precision:.2f}")
    assert precision >= floor
    assert np.allclose(val, np.sort(gv)[::-1], rtol=2e-3 if width == 20 else 1e-4)
    eng.close()


@pytest.mark.parametrize("width", [8, 16, 20, 21, 25, 26])
def test_narrow_fixed_point_travels_bit_packed(pkg, oracle, monkeypatch, width):
    """W <= 20 bits and <= 1024 columns: one dword per entry (20-bit value | 10-bit column | 2 flags), 4 B/nnz; W = 21..26 (the
    reference's 21-, 25- and 26-bit builds, test_spmv_topk.py:42-47): five bytes per entry (26 + 10 + 2 bits) -- the
    reference's reason for narrow types is more entries per transaction (types.hpp:57-79: B = 15 at 20 bits, 13 at 25, 11 at
    32). Same bits as the one-u32-per-value stream (TKSPMV_FIXED_UNPACKED=1) and as the integer model; wider words or more
    columns keep 6 B/nnz."""
    bpe = 4 if width <= 20 else 5
    import torch
    m = pkg.generate_matrix(120000, 1024, 20, "gamma", 12)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 40 + i) for i in range(4)])
    xs[1] *= np.float32(25.0)  # sums wrap at 2.0
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, precision=pkg.FIXED, fixed_width=width)
    info = eng.info()
    assert info["packed_bytes"] < (bpe + 0.1) * m.nnz + 8 * m.rows and info["packed_bytes"] > (bpe - 0.1) * m.nnz
    assert info["algorithmic_bytes"] == bpe * m.nnz + 4 * m.rows + (bpe - 2) * 1024 + 800
    monkeypatch.setenv("TKSPMV_FIXED_UNPACKED", "1")
    wide = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, precision=pkg.FIXED, fixed_width=width)
    monkeypatch.delenv("TKSPMV_FIXED_UNPACKED")
    assert wide.info()["packed_bytes"] > 5.9 * m.nnz
    for q in range(2):
        y, present = oracle.fixed_scores(m.row, m.col, m.val, xs[q], m.rows, width)
        ei, ev = oracle.select_topk(y, present, 100)
        for e in (eng, wide):
            e.reset(xs[q])
            e()
            val, idx = e.read_result()
            assert np.array_equal(idx, ei) and np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        assert np.array_equal(eng.scores().view(np.uint32), y.view(np.uint32))
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros(4, 100, dtype=torch.int32, device="cuda")
    out_v = torch.zeros(4, 100, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), 4, out_i.data_ptr(), out_v.data_ptr())  # the batch kernel on the packed stream
    eng.synchronize()
    for q in range(4):
        y, present = oracle.fixed_scores(m.row, m.col, m.val, xs[q], m.rows, width)
        ei, ev = oracle.select_topk(y, present, 100)
        assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), ei) and np.array_equal(out_v[q].cpu().numpy().view(np.uint32), ev.view(np.uint32))
    eng.close()
    wide.close()
    # 27 bits, or more than 1024 columns: one u32 per value + a column word
    for w, cols in ((27, 1024), (20, 3000), (25, 3000)):
        mm = pkg.generate_matrix(5000, cols, 20, "gamma", 3)
        e = pkg.SpMV(mm.row, mm.col, mm.val, mm.rows, mm.cols, k=10, device=0, precision=pkg.FIXED, fixed_width=w)
        assert e.info()["packed_bytes"] > 5.9 * mm.nnz
        e.close()
    # the packed stream round-trips through the packer's decoder and the .tkspmv file format
    p = pkg.Packed(m, k=100, nnz_per_lane=4, n_wave_partitions=4088, precision=pkg.FIXED, fixed_width=width)
    r, c, v = p.decode()
    assert np.array_equal(r, m.row) and np.array_equal(c, m.col)
    assert np.array_equal(v, np.minimum(np.floor(m.val.astype(np.float64) * 2 ** (width - 1)), 2 ** width - 1).astype(np.float32) / np.float32(2 ** (width - 1)))


def test_fixed_point_batch_equals_single_queries(pkg):
    import torch
    m = pkg.generate_matrix(70000, 1024, 20, "gamma", 31)
    nq = 5
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 900 + i) for i in range(nq)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, precision=pkg.FIXED, fixed_width=21,
                   stream_replicas=2)
    single = []
    for q in range(nq):
        eng.reset_device(dxs[q].data_ptr())
        eng()
        single.append(eng.read_result())
    out_i = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    for q in range(nq):
        val, idx = single[q]
        assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), idx), q
        assert np.array_equal(out_v[q].cpu().numpy(), val), q
    eng.close()


@pytest.mark.parametrize("rows,cols,nnz,k,seed", [(3000, 512, 40, 100, 1), (60000, 512, 40, 100, 2),
                                                  (20000, 1024, 20, 8, 3), (5000, 3000, 30, 50, 4), (5000, 6000, 30, 50, 5)])
def test_q1_7_wide_bit_exact_against_integer_model(pkg, oracle, rows, cols, nnz, k, seed):
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", seed)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, precision=pkg.Q1_7_WIDE)
    for q in range(2):
        x = pkg.create_sample_vector(cols, True, False, True, 10 * seed + q + 1)
        if q == 1:
            x = x * 0.01  # a different block scale
        eng.reset(x)
        eng()
        val, idx = eng.read_result()
        y, present, sh = oracle.q17_wide_scores(m.row, m.col, m.val, x, m.rows)
        assert sh > 0
        ei, ev = oracle.select_topk(y, present, k)
        assert np.array_equal(idx, ei), "index list differs from the integer model"
        assert np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        assert np.array_equal(eng.scores().view(np.uint32), y.view(np.uint32))
    eng.close()


def test_q1_7_wide_full_size_config_has_usable_precision(pkg, oracle):
    """BASELINE configs[4] shape with the wide-accumulation variant: bit-exact against its integer model and a
    precision@100 against the fp32 gold that is actually usable (the strict 8-bit variant scores 0.00 here)."""
    m = pkg.generate_matrix(1000000, 512, 40, "gamma", 5)
    x = pkg.create_sample_vector(512, True, False, True, 31)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=100, device=0, precision=pkg.Q1_7_WIDE)
    eng()
    val, idx = eng.read_result()
    y, present, sh = oracle.q17_wide_scores(m.row, m.col, m.val, x, m.rows)
    ei, ev = oracle.select_topk(y, present, 100)
    assert np.array_equal(idx, ei) and np.array_equal(val, ev)
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, x, 100)
    precision = len(set(idx.tolist()) & set(gi.tolist())) / 100.0
    print(f"Q1.7-wide precision@100 vs fp32 gold: {precision:.2f} (block scale 2^{sh})")
    assert precision >= 0.5
    assert np.allclose(val[0], gv[0], rtol=0.25)  # truncation at every step biases the scores low, uniformly
    eng.close()


# ---- multi-GPU exchange pieces that can be exercised on one GPU ------------------------------------------------------
def test_native_merge_kernel_matches_python_merge(pkg):
    import torch
    from importlib import import_module
    dmod = import_module("approximate_spmv_topk_amd.distributed")
    rng = np.random.RandomState(1)
    for world, k in ((2, 8), (4, 100), (8, 100), (8, 1000), (3, 7)):
        g = np.zeros((world, 2, k), dtype=np.int32)
        for r in range(world):
            n_real = k if r % 2 == 0 else max(1, k // 3)  # some shards return fillers
            sc = np.sort(rng.rand(n_real).astype(np.float32))[::-1]
            ids = (rng.permutation(10 * k)[:n_real] + r * 10 * k).astype(np.uint32)
            g[r, 0, :n_real] = ids.view(np.int32)
            g[r, 1, :n_real] = sc.view(np.int32)
        gt = torch.from_numpy(g).cuda()
        oi, ov = dmod.merge_topk_device(gt.reshape(-1), world, k)
        torch.cuda.synchronize()
        idx = (gt[:, 0, :].reshape(-1).to(torch.int64)) & 0xFFFFFFFF
        val = gt[:, 1, :].reshape(-1).contiguous().view(torch.float32)
        ei, ev = dmod.merge_candidates(idx, val, k)
        assert np.array_equal(oi.cpu().numpy().view(np.uint32).astype(np.int64), ei.cpu().numpy())
        assert np.array_equal(ov.cpu().numpy(), ev.cpu().numpy())


@pytest.mark.parametrize("multi_q", [0, 4])
@pytest.mark.parametrize("force_nccl", [False, True])
def test_native_sharded_step_single_rank(pkg, oracle, monkeypatch, force_nccl, multi_q):
    """world = 1: the pipelined native step (and, forced, a one-rank RCCL communicator with a real ncclAllGather)
    must return exactly what the engine returns, for a stream of queries."""
    import torch
    from importlib import import_module
    dmod = import_module("approximate_spmv_topk_amd.distributed")
    if force_nccl:
        monkeypatch.setenv("TKSPMV_DIST_FORCE_NCCL", "1")
    m = pkg.generate_matrix(80000, 1024, 20, "gamma", 17)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 900 + i) for i in range(6)])
    dxs = torch.from_numpy(xs).cuda()
    # multi_q = 4: the local step of an exchange batch runs as passes of four queries each
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, first_row=5000, multi_q=multi_q)
    nat = dmod.NativeShardedSpMV(eng, torch.device("cuda", 0))
    nat.set_batch(4)  # reads at q = 2 flush a partial batch, q = 5 lands in the middle of the next one
    for q in range(6):
        nat.enqueue(dxs[q].data_ptr())
        if q in (2, 5):  # read after a few pipelined queries: the result must be that of the LAST one
            val, idx = nat.read()
            gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[q], 100)
            assert set((idx - 5000).tolist()) == set(gi.tolist())
            assert np.allclose(val, gv, rtol=1e-4, atol=0)
    for batch in (1, 8, 32):
        nat.set_batch(batch)
        nat.run_many(dxs.data_ptr(), 6, 50)
        val, idx = nat.read()
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[49 % 6], 100)
        assert set((idx - 5000).tolist()) == set(gi.tolist())
    nat.close()
    eng.close()


# ---- several queries per pass over the matrix (tkspmv_enqueue_multi) -------------------------------------
@pytest.mark.parametrize("mq", [1, 2, 4, 8])
@pytest.mark.parametrize("rows,k,nq", [(70000, 100, 11), (1000000, 100, 9), (3000, 8, 5), (200000, 1, 4), (40000, 300, 6)])
def test_multi_query_passes_are_bit_identical_to_the_gold_order(pkg, oracle, mq, rows, k, nq):
    """The multi-query kernel sums every row in its own entry order -- the gold's sequential fp32 order; rows of more
    than 64 entries in segments of 64 -- so each query's list must equal, bit for bit, the exact selection over
    oracle_scores_f32_segmented. Groups of multi_q queries
    share a pass, the last group is partial, consecutive calls alternate the state-set halves; the one-query-per-pass
    path must agree with it on the index set (its scores follow the packet order: last-bit differences)."""
    import torch
    m = pkg.generate_matrix(rows, 1024, 20, "gamma", 77)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 300 + i) for i in range(nq)])
    xs[1] *= np.float32(0.01)  # queries of one pass with very different score scales: thresholds must not mix
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=2, multi_q=mq)
    # (8 queries per pass fall back to 4 when k exceeds a quarter of the threshold groups; above 3/8 the engine selects by
    # radix and has no multi-query kernel)
    ng = eng.info()["n_groups"]
    assert 8 * k <= 3 * ng and eng.info()["multi_q"] == (4 if mq == 8 and 4 * k > ng else mq)
    assert eng.info()["multi_bytes"] > 6 * m.nnz
    want = []
    for q in range(nq):
        y, present = oracle.scores_f32_segmented(m.row, m.col, m.val, xs[q], m.rows)
        want.append(oracle.select_topk(y, present, k))
    out_i = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
    for rep in range(3):
        out_i.fill_(-1)
        out_v.fill_(-1.0)
        eng.enqueue_multi(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        for q in range(nq):
            ei, ev = want[q]
            assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), ei), (rep, q)
            assert np.array_equal(out_v[q].cpu().numpy().view(np.uint32), ev.view(np.uint32)), (rep, q)
    # engine-owned buffers: the last query wins; the other entry points still work right after
    eng.enqueue_multi(dxs.data_ptr(), nq)
    val, idx = eng.read_result()
    assert np.array_equal(idx, want[nq - 1][0]) and np.array_equal(val, want[nq - 1][1])
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    eng.reset_device(dxs[0].data_ptr())
    eng()
    val, idx = eng.read_result()
    for q, (i_, v_) in ((2, (out_i[2].cpu().numpy().view(np.uint32), out_v[2].cpu().numpy())), (0, (idx, val))):
        ei, ev = want[q]
        if k < rows and len(np.unique(ev)) == k:
            assert len(set(i_.tolist()) ^ set(ei.tolist())) <= 2  # a K-th-boundary near-tie may swap
            assert np.allclose(np.sort(v_), np.sort(ev), rtol=1e-5)
    eng.close()


@pytest.mark.parametrize("precision", ["F32", "Q1_7_F32"])
@pytest.mark.parametrize("rows,passes", [(3000, None), (120000, None), (120000, "3"), (120000, "1"), (600000, None)])
def test_one_query_per_pass_launches_make_several_passes(pkg, oracle, precision, rows, passes):
    """multi_q = 1 (BASELINE configs[4]'s path): one launch of the row-per-lane kernel makes up to MULTI_PASSES passes, one query
    each, every pass with its own exchange-state set, x and result buffers; 37 queries = five launches on two chains, the
    last one partial. Every query's list equals the exact selection over the gold-order scores, bit for bit, whatever
    the number of passes per launch; a 3000-row matrix leaves most waves without a partition (they still meet the
    barriers of every pass)."""
    import torch
    nq, k, cols = 37, 50, 512
    m = pkg.generate_matrix(rows, cols, 40, "gamma", 91)
    vals = oracle.round_to_q17(m.val) if precision == "Q1_7_F32" else m.val
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 4100 + i) for i in range(nq)])
    xs[5] *= np.float32(0.01)
    xs[6] = -xs[6]
    dxs = torch.from_numpy(xs).cuda()
    if passes is not None:
        pkg.set_option("MULTI_PASSES", passes)
    try:
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=3, multi_q=1,
                       precision=getattr(pkg, precision), min_score=-100.0)
    finally:
        if passes is not None:
            pkg.set_option("MULTI_PASSES", None)
    assert eng.info()["multi_q"] == 1
    want = []
    for q in range(nq):
        y, present = oracle.scores_f32_segmented(m.row, m.col, vals, xs[q], m.rows)
        want.append(oracle.select_topk(y, present, k, min_score=-100.0))
    out_i = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
    for n in (nq, 8, 9, 1, 17):
        out_i.fill_(-1)
        out_v.fill_(-1.0)
        eng.enqueue_multi(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        for q in range(n):
            ei, ev = want[q]
            assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), ei), (n, q)
            assert np.array_equal(out_v[q].cpu().numpy().view(np.uint32), ev.view(np.uint32)), (n, q)
        assert int((out_i[n:] != -1).sum()) == 0
    eng.time_multi(dxs.data_ptr(), nq, 100)  # (the timing entry point: engine-owned result buffers, two launches in flight)
    eng.enqueue_multi(dxs.data_ptr(), 11)  # the engine-owned pair: the last query wins
    val, idx = eng.read_result()
    assert np.array_equal(idx, want[10][0]) and np.array_equal(val.view(np.uint32), want[10][1].view(np.uint32))
    eng.close()


def test_passes_that_drift_apart_still_find_their_thresholds(pkg, monkeypatch):
    """BASELINE configs[4]'s shape. The passes of a launch are not synchronised across workgroups: with the first workgroups
    as the only reducers and no second look at the passes they had left, a third of all timed runs went at 50 or 150 us per
    query instead of 18-19 (no threshold for most workgroups: every wave into its bounded wait, then a million candidates per
    query for the selection). Round 5: the guard is a COUNT
    (option STATS, tkspmv_debug_counters), not a wall clock: over twelve timed runs hardly any wave may have run into its bounded
    wait, and next to no row may have overflowed a list."""
    import torch
    monkeypatch.setenv("TKSPMV_STATS", "1")
    m = pkg.generate_matrix(1000000, 512, 40, "gamma", 5)
    xs = np.stack([pkg.create_sample_vector(512, True, False, True, 1000 + i) for i in range(16)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, precision=pkg.Q1_7_F32, multi_q=1, stream_replicas=4)
    waves = (eng.info()["grid"] - 8) * 8
    for _ in range(13):
        eng.time_multi(dxs.data_ptr(), 16, 512)
    c = eng.debug_counters()
    eng.close()
    nq = c["multi_stat_queries"]
    assert nq == 13 * 512, c
    # (the failure this guards against: ~every wave of ~every query in its wait, 10^5 .. 10^6 rows per query past the lists)
    assert c["multi_waits"] <= 0.02 * waves * nq, (c, waves)
    assert c["multi_rows_overflowed"] <= 5000 * nq, c  # (a few hundred per query: held slices judged before a threshold has arrived)
    print(f"\n[configs[4] shape, 13 x 512 queries] waits per query {c['multi_waits'] / nq:.2f} of {waves} waves, "
          f"{c['multi_wait_ticks'] * 0.01 / max(c['multi_waits'], 1):.2f} us each; rows offered {c['multi_rows_offered'] / nq:.0f}, overflowed {c['multi_rows_overflowed'] / nq:.2f} per query")


def test_multi_query_scores_are_the_reference_golds(pkg, oracle):
    """Against the gold itself (spmv_coo_gold_top_k + sort_tuples restated; the reference's own when oracle/_ref is
    present): same rows in the same order; score BITS equal for every row of at most 64 entries (longer rows are summed
    in segments: within 1e-6 relative)."""
    import torch
    m = pkg.generate_matrix(300000, 1024, 20, "gamma", 12)
    lens = np.bincount(m.row, minlength=m.rows)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 70 + i) for i in range(4)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, multi_q=4)
    out_i = torch.zeros((4, 100), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((4, 100), dtype=torch.float32, device="cuda")
    eng.enqueue_multi(dxs.data_ptr(), 4, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    n_bit_equal = 0
    for q in range(4):
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[q], 100)
        if oracle.have_ref():
            ri, rv = oracle.ref_gold_topk(m.row, m.col, m.val, xs[q], 100)
            assert np.array_equal(ri, gi) and np.array_equal(rv, gv)
        assert len(np.unique(gv)) == 100 and np.all(gv > 0)
        hi, hv = out_i[q].cpu().numpy().view(np.uint32), out_v[q].cpu().numpy()
        assert set(hi.tolist()) == set(gi.tolist())
        assert np.allclose(hv, gv, rtol=1e-6, atol=0)
        pos = {int(r): j for j, r in enumerate(gi)}
        for j, r in enumerate(hi):
            if lens[r] <= 64:
                assert hv[j].view(np.uint32) == gv[pos[int(r)]].view(np.uint32), (q, int(r))
                n_bit_equal += 1
    assert n_bit_equal >= 20  # (the best rows of a normalised matrix are mostly its long rows)
    eng.close()


def test_multi_query_edge_cases(pkg, oracle):
    """Signed values and negative min_score (lanes without a row must never surface), empty rows, k > rows, duplicates."""
    import torch
    rng = np.random.RandomState(3)
    lens = ([0, 3, 1, 0, 40, 300, 2, 7] * 40)[:-3]
    row = np.repeat(np.arange(len(lens)), lens).astype(np.uint32)
    col = rng.randint(0, 100, row.shape[0]).astype(np.uint32)
    val = (rng.rand(row.shape[0]).astype(np.float32) - np.float32(0.5))
    m = pkg.CooMatrix(len(lens), 100, row, col, val)
    xs = (rng.rand(3, 100).astype(np.float32) - np.float32(0.5))
    dxs = torch.from_numpy(xs).cuda()
    for k, min_score in ((16, -10.0), (400, -10.0), (16, 0.0)):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, multi_q=2, min_score=min_score)
        out_i = torch.zeros((3, k), dtype=torch.int32, device="cuda")
        out_v = torch.zeros((3, k), dtype=torch.float32, device="cuda")
        eng.enqueue_multi(dxs.data_ptr(), 3, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        for q in range(3):
            if eng.info()["multi_q"]:
                y, present = oracle.scores_f32_segmented(m.row, m.col, m.val, xs[q], m.rows)
                ei, ev = oracle.select_topk(y, present, k, min_score)
            else:  # (k = 400: selection by radix, no multi-query kernel: the ordinary sequence, packet-order sums)
                ei, ev = _expected(pkg, oracle, m, xs[q], k, eng, min_score)
            assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), ei), (k, min_score, q)
            assert np.array_equal(out_v[q].cpu().numpy().view(np.uint32), ev.view(np.uint32)), (k, min_score, q)
        eng.close()


def test_multi_query_falls_back_where_the_kernel_does_not_apply(pkg):
    """Wide x (or multi_q = 0): info.multi_q == 0 and enqueue_multi runs the ordinary sequence, same results as run()."""
    import torch
    m = pkg.generate_matrix(30000, 2000, 20, "gamma", 5)
    xs = np.stack([pkg.create_sample_vector(2000, True, False, True, 40 + i) for i in range(5)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=50, device=0, multi_q=4)
    assert eng.info()["multi_q"] == 0 and eng.info()["multi_bytes"] == 0
    out_i = torch.zeros((5, 50), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((5, 50), dtype=torch.float32, device="cuda")
    eng.enqueue_multi(dxs.data_ptr(), 5, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    for q in range(5):
        eng.reset_device(dxs[q].data_ptr())
        eng()
        val, idx = eng.read_result()
        assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), idx) and np.array_equal(out_v[q].cpu().numpy(), val)
    eng.close()
    with pytest.raises(pkg.TkspmvError):
        pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=50, device=0, multi_q=3)
    # Workgroups narrower than 512 threads: the multi-query kernel stages x with two words per thread, so 1024 columns
    # need 2 x blockDim >= 1024 -- such geometries must keep the ordinary sequence instead of scoring against unwritten LDS.
    m = pkg.generate_matrix(60000, 1024, 20, "gamma", 6)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 70 + i) for i in range(5)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=50, device=0, multi_q=4, threads_per_wg=256, waves_per_cu=4)
    assert eng.info()["multi_q"] == 0, eng.info()
    eng.enqueue_multi(dxs.data_ptr(), 5, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    for q in range(5):
        eng.reset_device(dxs[q].data_ptr())
        eng()
        val, idx = eng.read_result()
        assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), idx) and np.array_equal(out_v[q].cpu().numpy(), val)
    eng.close()


# ---- batches: the selection of query i rides inside the launch of query i+1 (deferred selection) ----------------------
@pytest.mark.parametrize("precision", ["F32", "Q1_7", "Q1_7_WIDE", "F16"])
@pytest.mark.parametrize("defer", ["1", "0"])
def test_batch_results_equal_single_query_results(pkg, oracle, monkeypatch, precision, defer):
    """tkspmv_enqueue_batch: every query of a batch must return bit for bit what the same query returns alone
    (fused single launch), whether its selection was deferred into the next launch, closed the batch, or the
    deferred scheme is switched off. Different x per query, so a mixed-up state set or result buffer shows."""
    import torch
    monkeypatch.setenv("TKSPMV_DEFER", defer)
    cols = 1024 if precision in ("F32", "F16") else 512
    m = pkg.generate_matrix(70000, cols, 20, "gamma", 31)
    nq = 7
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 700 + i) for i in range(nq)])
    if precision in ("Q1_7", "Q1_7_WIDE"):
        xs = (xs * np.float32(40.0)).astype(np.float32)  # keep Q1.7 scores away from all-zero
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, precision=getattr(pkg, precision),
                   stream_replicas=2)
    single = []
    for q in range(nq):
        eng.reset_device(dxs[q].data_ptr())
        eng()
        single.append(eng.read_result())
    out_i = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
    for rep in range(3):  # repeated batches: the two state sets keep alternating correctly across calls
        out_i.fill_(-1)
        eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        for q in range(nq):
            val, idx = single[q]
            assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), idx), (rep, q)
            assert np.array_equal(out_v[q].cpu().numpy(), val), (rep, q)
    # engine-owned buffers: last query wins; a single query right after a batch is still right
    eng.enqueue_batch(dxs.data_ptr(), nq)
    val, idx = eng.read_result()
    assert np.array_equal(idx, single[nq - 1][1]) and np.array_equal(val, single[nq - 1][0])
    eng.enqueue_many(dxs.data_ptr(), nq, 2 * nq + 3)
    val, idx = eng.read_result()
    assert np.array_equal(idx, single[(2 * nq + 2) % nq][1])
    eng.reset_device(dxs[1].data_ptr())
    eng()
    val, idx = eng.read_result()
    assert np.array_equal(idx, single[1][1]) and np.array_equal(val, single[1][0])
    if precision == "F32":
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[3], 100)
        assert set(single[3][1].tolist()) == set(gi.tolist())
    eng.close()


def test_long_batches_cross_launch_boundaries(pkg, oracle):
    """75 distinct queries through tkspmv_enqueue_batch = three launches of the batch kernel (32 + 32 + 11): every
    query bit-identical to its single-query result, and a sample of them identical to the oracle's packed-order model
    (scores) with the gold's top-K index set."""
    import torch
    m = pkg.generate_matrix(200000, 1024, 20, "gamma", 77)
    nq = 75
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 4000 + i) for i in range(nq)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, stream_replicas=2)
    out_i = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    bi = out_i.cpu().numpy().view(np.uint32)
    bv = out_v.cpu().numpy()
    for q in range(nq):
        assert np.all(bv[q][:-1] >= bv[q][1:]) and len(set(bi[q].tolist())) == 100, q
    for q in (0, 1, 31, 32, 33, 63, 64, 74):  # around the launch boundaries
        eng.reset_device(dxs[q].data_ptr())
        eng()
        val, idx = eng.read_result()
        assert np.array_equal(bi[q], idx) and np.array_equal(bv[q], val), q
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[q], 100)
        assert set(idx.tolist()) == set(gi.tolist()), q
        assert np.allclose(val, gv, rtol=RTOL, atol=0), q
    # the same batch again (state sets of all 32 queries are reused) gives the same bits
    out_i2 = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
    out_v2 = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i2.data_ptr(), out_v2.data_ptr())
    eng.synchronize()
    assert torch.equal(out_i, out_i2) and torch.equal(out_v, out_v2)
    eng.close()


@pytest.mark.parametrize("rows", [20000, 130000, 260000])
@pytest.mark.parametrize("precision,mode", [("F32", "1"), ("F32", "2"), ("Q1_7_WIDE", "2"), ("F16", "1")])
def test_workgroup_local_thresholds_are_verified_and_repaired(pkg, oracle, monkeypatch, rows, precision, mode):
    """TKSPMV_LOCAL=1/2: the threshold of a workgroup comes from its own waves (through LDS, no device-wide exchange), which proves
    nothing about the matrix as a whole: the selection verifies it, the repair launch re-runs what fails. 20 000 rows: few
    streaming waves per workgroup, whose best rows ARE the threshold -- with 100 results over a few hundred waves nearly
    every query fails the check and goes through the repair launch; 130 000 / 260 000 rows: the sizes the mode is for. All
    bit-identical to the device-wide exchange, and to the gold's index set."""
    import torch
    cols = 1024 if precision != "Q1_7_WIDE" else 512
    m = pkg.generate_matrix(rows, cols, 20, "gamma", 9)
    nq = 40
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 9100 + i) for i in range(nq)])
    if precision == "Q1_7_WIDE":
        xs = (xs * np.float32(40.0)).astype(np.float32)
    xs[7] = 0.0
    xs[8] = -xs[8]
    xs[20:24] *= np.float32(1e-2)
    dxs = torch.from_numpy(xs).cuda()
    kw = dict(k=100, device=0, precision=getattr(pkg, precision))
    monkeypatch.setenv("TKSPMV_LOCAL", "0")
    plain = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, **kw)
    ref_i = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
    ref_v = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
    plain.enqueue_batch(dxs.data_ptr(), nq, ref_i.data_ptr(), ref_v.data_ptr())
    plain.synchronize()
    plain.close()
    monkeypatch.setenv("TKSPMV_LOCAL", mode)  # (a wave's word: 1 = its best packet maximum, 2 = its second best)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, **kw)
    for rep in range(2):
        out_i = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
        out_v = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
        eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        bad = [q for q in range(nq) if not (torch.equal(out_i[q], ref_i[q]) and torch.equal(out_v[q], ref_v[q]))]
        assert not bad, (rep, bad)
    if precision == "F32":
        for q in (3, 21):
            gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[q], 100)
            assert set(out_i[q].cpu().numpy().view(np.uint32).tolist()) == set(gi.tolist()), q
    eng.close()


def test_local_thresholds_with_a_min_score_that_filters_most_rows(pkg, monkeypatch):
    """min_score above all but a few hundred rows' scores: most waves of a workgroup never see a row that counts, so most
    workgroups never form a local threshold (a wave's word needs a row above min_score). Results equal the device-wide
    exchange's bit for bit, fewer than k rows qualifying included, and no query may wait long for a threshold that cannot come
    (LOCAL_TAU_WAIT): the batch must not be slower than a few times the unfiltered one."""
    import torch
    m = pkg.generate_matrix(150000, 1024, 20, "gamma", 21)
    nq = 64
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 8800 + i) for i in range(nq)])
    dxs = torch.from_numpy(xs).cuda()
    base = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    bi = torch.zeros((nq, 100), dtype=torch.int32, device="cuda")
    bv = torch.zeros((nq, 100), dtype=torch.float32, device="cuda")
    base.enqueue_batch(dxs.data_ptr(), nq, bi.data_ptr(), bv.data_ptr())
    base.synchronize()
    t_plain = base.time_queries(dxs.data_ptr(), nq, 256)
    base.close()
    kth = float(np.sort(bv[0].cpu().numpy())[::-1][99])  # the 100th best score of the first query
    for frac_kept, factor in ((3.0, 0.93), (0.4, 1.12)):  # min_score a little below / above it: a few hundred / fewer than k rows qualify
        min_score = kth * factor
        res = {}
        for mode in ("0", "auto"):
            if mode == "0":
                monkeypatch.setenv("TKSPMV_LOCAL", "0")
            else:
                monkeypatch.delenv("TKSPMV_LOCAL", raising=False)
            eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0, min_score=min_score)
            oi = torch.full((nq, 100), -1, dtype=torch.int32, device="cuda")
            ov = torch.full((nq, 100), -1.0, dtype=torch.float32, device="cuda")
            eng.enqueue_batch(dxs.data_ptr(), nq, oi.data_ptr(), ov.data_ptr())
            eng.synchronize()
            res[mode] = (oi.clone(), ov.clone(), eng.time_queries(dxs.data_ptr(), nq, 256), eng.info()["batch_mode"])
            eng.close()
        assert (res["auto"][3] >> 8) & 0xFF != 0 and (res["0"][3] >> 8) & 0xFF == 0
        assert torch.equal(res["0"][0], res["auto"][0]) and torch.equal(res["0"][1], res["auto"][1]), frac_kept
        assert res["auto"][2] < 3.0 * t_plain, (res["auto"][2], t_plain)
        if frac_kept < 1:
            assert int((res["auto"][1][0] == 0).sum()) > 0  # (fewer than k rows qualify: the lists are padded like the reference's)


def test_local_thresholds_switch_themselves_off_on_adversarial_data(pkg, monkeypatch):
    """What defeats the 8 slots of a workgroup is a matrix whose best rows sit, a few each, in ALL the partitions of the same
    workgroups (many in ONE partition are harmless: that wave hands them over itself). Built here from the engine's own cut:
    five heavy rows at the head of each of the 8 partitions of three workgroups -- 120 rows that hold every top-100, 40 per
    workgroup. Every check fails, whatever the thresholds do. Results stay exact (the repair launch), and the mode must not
    keep paying for it: a launch of which a quarter failed closes the gate for 8, 16, ... launches (tkspmv_debug_counters)."""
    import torch
    m = pkg.generate_matrix(200000, 1024, 20, "gamma", 13)
    probe = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    info = probe.info()
    probe.close()
    n_wg = info["grid"] - (info["batch_mode"] & 0xFF)
    assert (info["batch_mode"] >> 8) & 0xFF != 0  # local thresholds are this size's default
    packed = pkg.Packed(m, k=100, nnz_per_lane=4, n_wave_partitions=info["batch_mode"] >> 16)
    _, _, pkt_row, part_first, _ = packed.raw()
    assert len(part_first) == info["n_wave_partitions"] and len(part_first) > 7 * n_wg + 200
    heavy = np.concatenate([pkt_row[part_first[b + w * n_wg]] + np.arange(5) for b in (3, 77, 200) for w in range(8)])
    val = m.val.copy()
    val[np.isin(m.row, heavy)] *= np.float32(50.0)
    nq, launches = 64, 12
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 7700 + i) for i in range(nq)])
    dxs = torch.from_numpy(np.tile(xs, (launches * 32 // nq, 1))).cuda()
    total = dxs.shape[0]
    monkeypatch.setenv("TKSPMV_LOCAL", "0")
    plain = pkg.SpMV(m.row, m.col, val, m.rows, m.cols, k=100, device=0)
    ref_i = torch.full((total, 100), -1, dtype=torch.int32, device="cuda")
    ref_v = torch.full((total, 100), -1.0, dtype=torch.float32, device="cuda")
    plain.enqueue_batch(dxs.data_ptr(), total, ref_i.data_ptr(), ref_v.data_ptr())
    plain.synchronize()
    assert plain.debug_counters()["checks_failed"] == 0
    plain.close()
    assert bool(np.isin(ref_i.cpu().numpy().view(np.uint32), heavy).all())  # (the premise: every result row is a heavy row)
    monkeypatch.delenv("TKSPMV_LOCAL")
    eng = pkg.SpMV(m.row, m.col, val, m.rows, m.cols, k=100, device=0)
    out_i = torch.full((total, 100), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((total, 100), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), total, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    assert torch.equal(out_i, ref_i) and torch.equal(out_v, ref_v)
    c = eng.debug_counters()
    assert c["batch_launches"] == launches
    # launch 1 fails throughout and closes the gate for 8 launches; launch 10 tries again, fails, closes it for 16
    assert c["checks_failed"] == 64 and c["local_off_length"] == 16 and c["local_off_for_launches"] == 14, c
    eng.close()


@pytest.mark.parametrize("cols,k", [(4096, 100), (1024, 600), (16384, 10)])
def test_batches_on_geometries_without_the_batch_kernel(pkg, oracle, cols, k):
    """x too large to sit twice in LDS, or K above the number of publishing workgroups (several groups per workgroup /
    exchange off): sequences fall back to one launch per query; results must not care."""
    import torch
    m = pkg.generate_matrix(30000, cols, 20, "gamma", 5)
    nq = 5
    xs = np.stack([pkg.create_sample_vector(cols, True, False, True, 300 + i) for i in range(nq)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    out_i = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), nq, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    for q in range(nq):
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[q], k)
        got = out_i[q].cpu().numpy().view(np.uint32)
        assert set(got.tolist()) == set(gi.tolist()), q
        assert np.allclose(out_v[q].cpu().numpy(), gv, rtol=RTOL, atol=0), q
    eng.close()


# ---- packed-matrix cache: an engine created from a .tkspmv file ------------------------------------------------------
@pytest.mark.parametrize("precision", ["F32", "Q1_7_WIDE"])
def test_engine_from_packed_file_equals_engine_from_coo(pkg, oracle, tmp_path, precision):
    import time
    m = pkg.generate_matrix(150000, 1024 if precision == "F32" else 512, 20, "gamma", 12)
    x = pkg.create_sample_vector(m.cols, True, False, True, 77)
    if precision != "F32":
        x = (x * np.float32(30.0)).astype(np.float32)
    prec = getattr(pkg, precision)
    t0 = time.perf_counter()
    a = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x, k=100, device=0, precision=prec)
    t_coo = time.perf_counter() - t0
    a()
    va, ia = a.read_result()
    n_parts = pkg.Packed.wave_partitions(device=0, m=m, precision=prec)
    # one partition per streaming wave; workgroup 0 -- on small matrices workgroups 0..3 -- left to the selection
    assert n_parts == (a.info()["grid"] - max(a.info()["batch_mode"] & 0xFF, 1)) * 8 == a.info()["batch_mode"] >> 16
    assert pkg.Packed.wave_partitions(device=0) == a.info()["grid"] * 8 - 8  # (matrix unknown: the most any engine accepts)
    packed = pkg.Packed(m, k=100, n_wave_partitions=n_parts, precision=pkg.F32 if precision == "F32" else pkg.Q1_7)
    path = tmp_path / "m.tkspmv"
    packed.save(path)
    t0 = time.perf_counter()
    b = pkg.SpMV.from_packed(pkg.Packed.load(path), k=100, vec=x, device=0, precision=prec)
    t_file = time.perf_counter() - t0
    b()
    vb, ib = b.read_result()
    claim = a.info()["claim_sets"] != 0  # fp32: tkspmv_create cuts sets of 8 partitions that workgroups claim (other packet cuts)
    assert np.array_equal(ia, ib) and (np.allclose(va, vb, rtol=1e-5, atol=0) if claim else np.array_equal(va, vb))
    if not claim:
        assert a.info()["n_packets"] == b.info()["n_packets"] and a.info()["n_wave_partitions"] == b.info()["n_wave_partitions"]
    print(f"setup from COO {t_coo * 1e3:.1f} ms, from the packed file {t_file * 1e3:.1f} ms")
    # a file packed for a bigger launch geometry is refused -- unless the engine deals partitions out dynamically --, a smaller
    # one works (idle waves)
    big = pkg.Packed(m, k=100, n_wave_partitions=2 * n_parts, precision=pkg.F32 if precision == "F32" else pkg.Q1_7)
    if big.info()["n_wave_partitions"] > n_parts:
        if claim:
            e2 = pkg.SpMV.from_packed(big, k=100, vec=x, device=0, precision=prec)
            e2()
            v2, i2 = e2.read_result()
            assert np.array_equal(ia, i2) and np.allclose(va, v2, rtol=1e-5, atol=0)
            e2.close()
        else:
            with pytest.raises(pkg.TkspmvError) as ei:
                pkg.SpMV.from_packed(big, k=100, device=0, precision=prec)
            assert ei.value.status == pkg._lib.ERR_UNSUPPORTED
    small = pkg.Packed(m, k=100, n_wave_partitions=n_parts // 3, precision=pkg.F32 if precision == "F32" else pkg.Q1_7)
    c = pkg.SpMV.from_packed(small, k=100, vec=x, device=0, precision=prec)
    c()
    vc, ic = c.read_result()
    assert np.array_equal(ia, ic)  # same rows, same order; the sums may differ in the last bit (other packet cuts)
    assert np.allclose(va, vc, rtol=1e-5, atol=0)
    for e in (a, b, c):
        e.close()


def test_three_million_rows(pkg, oracle):
    """Beyond BASELINE configs[1]: 3M x 1024 (58M nnz, 0.35 GB packed, 56 packets per wave partition) -- the size one
    GPU holds of configs[3] with room to spare. Single query against the CPU gold; a batch against the single queries."""
    import torch
    m = pkg.generate_matrix(3000000, 1024, 20, "gamma", 21)
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 8000 + i) for i in range(3)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    info = eng.info()
    assert info["nnz"] == m.row.shape[0] and info["packets_per_partition"] * info["packet_entries"] >= 50 * 256
    singles = []
    for q in range(3):
        eng.reset_device(dxs[q].data_ptr())
        eng()
        singles.append(eng.read_result())
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, xs[0], 100)
    assert set(singles[0][1].tolist()) == set(gi.tolist())
    assert np.allclose(singles[0][0], gv, rtol=RTOL, atol=0)
    out_i = torch.zeros(3, 100, dtype=torch.int32, device="cuda")
    out_v = torch.zeros(3, 100, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), 3, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    for q in range(3):
        assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), singles[q][1])
        assert np.array_equal(out_v[q].cpu().numpy(), singles[q][0])
    ns = eng.time_queries(dxs.data_ptr(), 3, 64)
    print(f"3M rows: {ns / 1e3:.1f} us per query, {info['algorithmic_bytes'] / ns:.0f} GB/s algorithmic")
    eng.close()


# ---- TKSPMV_F16: fp16 values, fp32 x and arithmetic (the CUDA comparator's -a mode) -----------------------------------
@pytest.mark.parametrize("rows,cols,nnz,k,seed", [(3000, 512, 40, 100, 1), (120000, 1024, 20, 100, 2), (20000, 3000, 30, 8, 3),
                                                  (5000, 6000, 30, 50, 5)])
def test_f16_values_bit_exact_against_the_half_model(pkg, oracle, rows, cols, nnz, k, seed):
    """Bit-exact against the order-matched oracle reading the same 2-byte value stream; and, against the fp32 gold,
    the ranking quality the reference reports for its half mode: high precision@K, scores within fp16 rounding."""
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", seed)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, precision=pkg.F16)
    info = eng.info()
    assert info["packet_entries"] == 256 and info["packed_bytes"] < 4.1 * m.row.shape[0] + 8 * rows + 70000
    packed = pkg.Packed(m, k=k, n_wave_partitions=pkg.Packed.wave_partitions(0, m=m, precision=pkg.F16), precision=pkg.F16)
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    for q in range(2):
        x = pkg.create_sample_vector(cols, True, False, True, 50 * seed + q)
        eng.reset(x)
        eng()
        val, idx = eng.read_result()
        yp, present = oracle.packed_scores(packed.raw(), x, m.rows, 4)
        ei, ev = oracle.select_topk(yp, present, k)
        assert np.array_equal(idx, ei), "index list differs from the half-value oracle"
        assert np.array_equal(val.view(np.uint32), ev.view(np.uint32)), "scores are not bit-identical"
        assert np.array_equal(eng.scores().view(np.uint32), yp.view(np.uint32))
        # the same thing said differently: the fp32 gold over values rounded to half
        gi_h, gv_h = oracle.gold_topk(m.row, m.col, oracle.round_to_half(m.val), x, k)
        assert len(set(idx.tolist()) & set(gi_h.tolist())) >= k - 1 and np.allclose(val, gv_h, rtol=1e-4, atol=0)
        gi, gv = oracle.gold_topk(m.row, m.col, m.val, x, k)
        prec = len(set(idx.tolist()) & set(gi.tolist())) / k
        assert prec >= 0.9, prec
        assert np.allclose(val, gv, rtol=2e-3, atol=0)
    eng.close()


def test_batch_corner_counts_and_a_long_run(pkg, oracle):
    """count = 0 and 1, counts around the launch size, and 20 000 queries in one call (625 launches of the batch kernel:
    tickets, state sets and the replica rotation keep cycling) -- the last result must still be the right one."""
    import torch
    m = pkg.generate_matrix(40000, 1024, 20, "gamma", 3)
    nx = 5
    xs = np.stack([pkg.create_sample_vector(1024, True, False, True, 600 + i) for i in range(nx)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=50, device=0, stream_replicas=3)
    single = []
    for q in range(nx):
        eng.reset_device(dxs[q].data_ptr())
        eng()
        single.append(eng.read_result())
    eng.enqueue_batch(dxs.data_ptr(), 0)
    eng.synchronize()
    for count in (1, 2, 31, 32, 33, 64, 65):
        eng.enqueue_many(dxs.data_ptr(), nx, count)
        val, idx = eng.read_result()
        assert np.array_equal(idx, single[(count - 1) % nx][1]) and np.array_equal(val, single[(count - 1) % nx][0]), count
    eng.enqueue_many(dxs.data_ptr(), nx, 20000)
    val, idx = eng.read_result()
    assert np.array_equal(idx, single[(20000 - 1) % nx][1]) and np.array_equal(val, single[(20000 - 1) % nx][0])
    eng.close()


def test_multi_query_small_counts_and_k_above_the_publishing_groups(pkg, oracle):
    """count = 0 and 1; k too large for a threshold to form (exchange off: no multi-query kernel, the sequence runs)."""
    import torch
    m = pkg.generate_matrix(50000, 512, 20, "uniform", 9)
    xs = np.stack([pkg.create_sample_vector(512, True, False, True, 5 + i) for i in range(2)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=10, device=0, multi_q=8)
    out_i = torch.full((2, 10), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((2, 10), -1.0, dtype=torch.float32, device="cuda")
    eng.enqueue_multi(dxs.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    assert int(out_i.min()) == -1 and int(out_i.max()) == -1
    eng.enqueue_multi(dxs.data_ptr(), 1, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    y, present = oracle.scores_f32_segmented(m.row, m.col, m.val, xs[0], m.rows)
    ei, ev = oracle.select_topk(y, present, 10)
    assert np.array_equal(out_i[0].cpu().numpy().view(np.uint32), ei) and np.array_equal(out_v[0].cpu().numpy(), ev)
    assert int(out_i[1].max()) == -1
    eng.close()
    big = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=1024, device=0, multi_q=4)
    if big.info()["n_groups"] == 0:  # fewer publishing groups than k
        assert big.info()["multi_q"] == 0
    oi = torch.zeros((2, 1024), dtype=torch.int32, device="cuda")
    ov = torch.zeros((2, 1024), dtype=torch.float32, device="cuda")
    big.enqueue_multi(dxs.data_ptr(), 2, oi.data_ptr(), ov.data_ptr())
    big.synchronize()
    v = ov[1].cpu().numpy()
    assert np.all(v[:-1] >= v[1:]) and len(set(oi[1].cpu().numpy().tolist())) == 1024
    big.close()


# ---- large k: scores + radix select -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [400, 1000, 1023, 1024])
@pytest.mark.parametrize("rows,cols,nnz,seed", [(200000, 1024, 20, 3), (1500, 64, 6, 4), (60000, 3000, 30, 5)])
def test_large_k_radix_select_path(pkg, oracle, k, rows, cols, nnz, seed):
    """k above 3/8 of the publishing groups (or above all of them: no threshold can form): the engine scores every row and
    selects by radix. Bit-exact against the packed-order oracle + exact selection, min_score respected, k > rows padded."""
    m = pkg.generate_matrix(rows, cols, nnz, "gamma", seed)
    for min_score in (0.0, 0.05):
        eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, min_score=min_score)
        for q in range(2):
            x = pkg.create_sample_vector(cols, True, False, True, 20 * seed + q)
            eng.reset(x)
            eng()
            val, idx = eng.read_result()
            ei, ev = _expected(pkg, oracle, m, x, k, eng, min_score)
            assert np.array_equal(idx, ei), (k, min_score, q)
            assert np.array_equal(val.view(np.uint32), ev.view(np.uint32))
        eng.close()


def test_large_k_radix_select_ties_and_batches(pkg, oracle):
    """Massive ties at the k-th score (all values 1, -v mode: scores are small integers) and the batch entry points."""
    import torch
    m = pkg.generate_matrix(50000, 256, 6, "uniform", 2)
    ones = np.ones_like(m.val)
    xs = np.stack([np.full(256, 0.5, dtype=np.float32), pkg.create_sample_vector(256, True, False, True, 9)])
    dxs = torch.from_numpy(xs).cuda()
    eng = pkg.SpMV(m.row, m.col, ones, m.rows, m.cols, k=800, device=0)
    out_i = torch.zeros((2, 800), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((2, 800), dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), 2, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    mm = pkg.CooMatrix(m.rows, m.cols, m.row, m.col, ones)
    for q in range(2):
        ei, ev = _expected(pkg, oracle, mm, xs[q], 800, eng)
        assert np.array_equal(out_i[q].cpu().numpy().view(np.uint32), ei) and np.array_equal(out_v[q].cpu().numpy(), ev)
    eng.close()


def test_degenerate_queries_every_row_a_candidate(pkg, oracle):
    """x = 0 (every score 0.0 = min_score: every row is a candidate and ties with every other) and all-equal positive scores
    (identical rows): the exact list by (score desc, row desc) -- the k LARGEST row ids -- through the fused single launch and
    through the batch kernel, alone and between ordinary queries (the reference's gold keeps whichever tied rows its
    insertion order favours, gold_algorithms.hpp:219-230; this engine's contract is the total order of sort_tuples)."""
    import torch
    k, rows = 100, 200000
    m = pkg.generate_matrix(rows, 1024, 20, "gamma", 6)
    x0 = np.zeros(1024, np.float32)
    xr = pkg.create_sample_vector(1024, True, False, True, 61)
    eng = pkg.SpMV(m.row, m.col, m.val, m.rows, m.cols, vec=x0, k=k, device=0)
    eng()
    val, idx = eng.read_result()
    present = np.zeros(rows, bool)
    present[m.row] = True
    want = np.flatnonzero(present)[::-1][:k].astype(np.uint32)  # rows that own an entry, largest ids first
    assert np.array_equal(idx, want) and np.all(val == 0.0)
    # the same through the batch kernel: zero vectors between ordinary queries (their lists must be untouched by the flood)
    xs = np.stack([xr, x0, x0, xr, x0])
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros(5, k, dtype=torch.int32, device="cuda")
    out_v = torch.zeros(5, k, dtype=torch.float32, device="cuda")
    eng.enqueue_batch(dxs.data_ptr(), 5, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    oi, ov = out_i.cpu().numpy().astype(np.uint32), out_v.cpu().numpy()
    gi, gv = oracle.gold_topk(m.row, m.col, m.val, xr, k)
    for q in (1, 2, 4):
        assert np.array_equal(oi[q], want) and np.all(ov[q] == 0.0)
    for q in (0, 3):
        assert set(oi[q].tolist()) == set(gi.tolist()) and np.allclose(ov[q], gv, rtol=1e-4, atol=0)
    eng.close()
    # identical rows: one entry of value 0.5 in column 3 per row, x[3] = 2 -> every score is exactly 1.0
    rows2 = 150000
    r = np.arange(rows2, dtype=np.uint32)
    c = np.full(rows2, 3, np.uint32)
    v = np.full(rows2, 0.5, np.float32)
    x1 = np.zeros(1024, np.float32)
    x1[3] = 2.0
    eng = pkg.SpMV(r, c, v, rows2, 1024, vec=x1, k=k, device=0)
    eng()
    val, idx = eng.read_result()
    assert np.array_equal(idx, np.arange(rows2 - 1, rows2 - 1 - k, -1, dtype=np.uint32)) and np.all(val == 1.0)
    eng.close()
