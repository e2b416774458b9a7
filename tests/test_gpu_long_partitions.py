"""Long partitions: engines created from a prepacked matrix (SpMV.from_packed(Packed(m, n_wave_partitions=P))) whose partitions hold
63 .. 3055 packets -- the default engines of the fast tests stop at about 20. What depends on a partition's length: the batch kernel
of local thresholds and single_kernel keep the packets' row bases in lanes up to 64 packets and load them beyond; the timetable books
a packet's slot as period / packets; the range, facet, match and filtered kernels walk the row table on their candidate path and
flush a per-wave list of 256 entries; fewer partitions than k leave the device-wide threshold unformed; the row lookup bisects the
partition table.

The order-matched oracle reads packed.raw() of the very Packed object the engine was created from (for a prepacked engine
batch_mode >> 16 is the launch geometry's wave count, not the partition count). Every top-k list is compared bit for bit with it and
through _exact with the fp64 gold. The partition lengths below were checked with the host packer; every test asserts them again.
The conftest syncs torch only for the existing enqueue names: these tests call torch.cuda.synchronize() themselves."""
import numpy as np
import pytest

import support
from support import bits
from test_gpu_range import _Dev, _check_query, _expected, _thresholds
from test_gpu_single import _exact

pytestmark = pytest.mark.gpu

FIRST = {49: 63, 48: 64, 47: 66, 8: 382, 1: 3055}  # generate_matrix(40000, 1024, 20, "gamma", 41): partitions -> packets per partition
SECOND = {49: 64, 48: 65}                          # generate_matrix(20000, 512, 40, "gamma", 42)
COUNTERS = ("checks_failed", "single_launches", "single_repairs", "batch_launches", "late_repairs")


class _Shape:
    def __init__(self, pkg, rows, cols, nnz, seed, n_q, x_seed):
        self.m = pkg.generate_matrix(rows, cols, nnz, "gamma", seed)
        self.xs = np.stack([pkg.create_sample_vector(cols, True, False, True, x_seed + i) for i in range(n_q)]).astype(np.float32)


@pytest.fixture(scope="module")
def first(pkg):
    return _Shape(pkg, 40000, 1024, 20, 41, 16, 4100)


@pytest.fixture(scope="module")
def second(pkg):
    return _Shape(pkg, 20000, 512, 40, 42, 8, 4200)


def _pack(pkg, m, P, want, k, **kw):
    packed = pkg.Packed(m, k=k, n_wave_partitions=P, **kw)
    info = packed.info()
    assert info["n_wave_partitions"] == P and info["packets_per_partition"] == want[P], info
    return packed


def _prepacked(pkg, packed, k, **kw):
    eng = pkg.SpMV.from_packed(packed, k=k, device=0, **kw)
    info, pinfo = eng.info(), packed.info()
    assert info["n_wave_partitions"] == pinfo["n_wave_partitions"] and info["packets_per_partition"] == pinfo["packets_per_partition"], info
    return eng, info


def _some(c):
    return {key: c[key] for key in COUNTERS}


def _run(eng, x):
    eng.reset(x)
    assert eng() > 0
    return eng.read_result()


def _batch_lists(eng, xs, k):
    """One enqueue_batch of the rows of xs with per-query buffers: (idx[n, k] uint32, val[n, k])."""
    import torch
    n = xs.shape[0]
    dxs = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    out_i = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    out_v = torch.full((n, k), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    return out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy()


def _served(before, after, n):
    """Which path served n tkspmv_run calls: single_kernel (every call counts a launch) or the stream kernel (none does)."""
    d = after["single_launches"] - before["single_launches"]
    assert d in (0, n), f"{d} single_kernel launches for {n} tkspmv_run calls"
    return "single" if d == n else "stream"


# ---- 1. the 64-packet boundary under local thresholds ---------------------------------------------------------------------------
@pytest.mark.parametrize("local", ["1", "2"])
@pytest.mark.parametrize("k", [8, 100])
@pytest.mark.parametrize("P", [49, 48, 47])
def test_boundary_local_thresholds(pkg, oracle, monkeypatch, first, P, k, local):
    """63 / 64 / 66 packets per partition with TKSPMV_LOCAL forced (the failure estimate switches local thresholds off at this few
    partitions): 6 queries and the -x of the last through tkspmv_run, then 12 queries (one of them the -x of its predecessor) through
    the batch kernel. Repairs are allowed, wrong lists are not.
    KEEP [47-8-2] (P = 47, k = 8, LOCAL = 2): at 47 .. 49 partitions most checks of the local kernels fail and the exact launch
    answers instead (6 of 7 runs and 11 of 12 batch queries repaired in the other cases), so a list that the local kernels computed
    THEMSELVES over a partition of more than 64 packets is delivered often enough only there (2 of 7 runs, 3 of 12 batch queries
    repaired). With `np <= 64u` changed to `<= 66u` in batch_kernel.hpp, or in local.hpp, that case alone fails."""
    monkeypatch.setenv("TKSPMV_LOCAL", local)
    m, xs = first.m, first.xs
    packed = _pack(pkg, m, P, FIRST, k)
    eng, info = _prepacked(pkg, packed, k)
    assert info["batch_mode"] & 0xFF, "the batch kernel is expected to serve this engine"
    assert (info["batch_mode"] >> 8) & 0xFF == int(local), info
    raw, C = packed.raw(), info["packet_entries"] // 64
    c0 = eng.debug_counters()
    for q in range(6):
        val, idx = _run(eng, xs[q])
        _exact(pkg, oracle, m, eng, xs[q], k, idx, val, raw, C)
    x = (xs[5] * np.float32(-1.0)).astype(np.float32)  # (no row reaches a threshold carried from +x: the check fails by sign)
    val, idx = _run(eng, x)
    _exact(pkg, oracle, m, eng, x, k, idx, val, raw, C, gold=False)
    c1 = eng.debug_counters()
    served = _served(c0, c1, 7)
    if served == "single":
        assert c1["single_repairs"] == c1["single_checks_failed"], c1
    xb = xs[4:16].copy()
    xb[7] = xb[6] * np.float32(-1.0)
    bi, bv = _batch_lists(eng, xb, k)
    for q in range(12):
        _exact(pkg, oracle, m, eng, xb[q], k, bi[q], bv[q], raw, C, gold=q != 7)
    c2 = eng.debug_counters()
    assert c2["batch_launches"] > c1["batch_launches"], c2
    print(f"\n[P={P}: {FIRST[P]} packets per partition, k={k}, LOCAL={local}] tkspmv_run served by {served}; grid {info['grid']} x {info['block']}, "
          f"batch_mode {info['batch_mode']:#x}; after 7 runs {_some(c1)}; after the batch of 12 {_some(c2)}")
    eng.close()


# ---- 2. the exact exchange with fewer partitions than k -------------------------------------------------------------------------
@pytest.mark.parametrize("P", [49, 48, 47])
def test_boundary_exact_exchange_with_fewer_partitions_than_k(pkg, oracle, monkeypatch, first, P):
    """TKSPMV_LOCAL=0, k = 100 on 47 .. 49 partitions: fewer groups publish a maximum than the threshold needs, it never forms and
    every row goes through the slots and the overflow lists."""
    monkeypatch.setenv("TKSPMV_LOCAL", "0")
    k = 100
    m, xs = first.m, first.xs
    packed = _pack(pkg, m, P, FIRST, k)
    assert P < k
    eng, info = _prepacked(pkg, packed, k)
    assert info["batch_mode"] & 0xFF and (info["batch_mode"] >> 8) & 0xFF == 0, info
    raw, C = packed.raw(), info["packet_entries"] // 64
    c0 = eng.debug_counters()
    bi, bv = _batch_lists(eng, xs[:12], k)
    for q in range(12):
        _exact(pkg, oracle, m, eng, xs[q], k, bi[q], bv[q], raw, C)
    c1 = eng.debug_counters()
    assert c1["batch_launches"] > c0["batch_launches"] and c1["checks_failed"] == 0, c1
    print(f"\n[P={P}: {FIRST[P]} packets per partition, k={k}, LOCAL=0] batch exact; n_groups {info['n_groups']}, batch_mode {info['batch_mode']:#x}; {_some(c1)}")
    eng.close()


# ---- 3. very long partitions: every query form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [8, 1])
def test_very_long_partitions_every_query_form(pkg, oracle, first, P):
    """382 and 3055 packets per partition, k = 100: tkspmv_run, a batch, the scores of every row, range queries down to threshold 0
    (one wave's list flushed more than 150 times at P = 1), filtered, facet, grouped, search-after and match queries, and the row
    lookup of score_rows / row_vectors at the first and last row of every partition. An fp32 engine refuses none of these forms:
    a TkspmvError fails the test."""
    import torch
    k = 100
    m, xs = first.m, first.xs
    rows, x = m.rows, xs[0]
    packed = _pack(pkg, m, P, FIRST, k)
    eng, info = _prepacked(pkg, packed, k)
    raw, C = packed.raw(), info["packet_entries"] // 64
    yp, present = oracle.packed_scores(raw, x, rows, C)
    present = present.astype(bool)
    ones = np.ones(rows, dtype=bool)

    # tkspmv_run, the scores of every row, a batch of 5
    c0 = eng.debug_counters()
    val, idx = _run(eng, x)
    _exact(pkg, oracle, m, eng, x, k, idx, val, raw, C)
    c1 = eng.debug_counters()
    served = _served(c0, c1, 1)
    assert np.array_equal(bits(eng.scores()), bits(yp)), "tkspmv_scores differs from the order-matched oracle"
    bi, bv = _batch_lists(eng, xs[1:6], k)
    for q in range(5):
        _exact(pkg, oracle, m, eng, xs[1 + q], k, bi[q], bv[q], raw, C)
    c2 = eng.debug_counters()

    # range queries: _thresholds' ladder and 0.0 (every row with entries)
    thr = _thresholds(yp, present, [("zero", 0.0)])
    names = list(thr)
    tv = np.array([thr[n] for n in names], dtype=np.float32)
    exps = [_expected(yp, present, ones, t) for t in tv]
    assert len(exps[names.index("zero")]) == int(present.sum()) > 150 * 256 // P  # (full lists of 256 rows per wave and query)
    cap = max(len(e) for e in exps)
    dev = _Dev(torch, len(names), cap)
    dthr = torch.from_numpy(tv).cuda()
    dxs = torch.from_numpy(np.tile(x, (len(names), 1))).cuda()
    torch.cuda.synchronize()
    eng.enqueue_range(dxs.data_ptr(), len(names), dthr.data_ptr(), dev.counts.data_ptr(), dev.idx.data_ptr(), dev.val.data_ptr(), cap)
    eng.synchronize()
    counts, gi, gv = dev.host()
    for i, name in enumerate(names):
        _check_query(counts[i], gi[i], gv[i], cap, exps[i], f"P={P}/range/{name}")
    for name in ("rank100", "zero"):
        rv, ri = eng.run_range(thr[name])
        exp = exps[names.index(name)]
        ei, ev = oracle.sort_tuples(np.array([r for r, _ in exp], dtype=np.uint32), np.array([b for _, b in exp], dtype=np.uint32).view(np.float32))
        assert eng.last_range_count == len(exp) and np.array_equal(ri, ei) and np.array_equal(bits(rv), bits(ev)), f"P={P}/run_range/{name}"

    # filtered top-k under a dense and a very sparse mask
    masks = support.masks(rows, idx, 0, rows)
    dx = torch.from_numpy(x).cuda()
    for name in ("random0.5", "random0.001"):
        allow = masks[name]
        dmask = torch.from_numpy(pkg.row_mask(rows, allow).view(np.int32)).cuda()
        out_i = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        out_v = torch.full((k,), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.enqueue_filtered(dx.data_ptr(), 1, dmask.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr())
        eng.synchronize()
        ei, ev = oracle.select_topk(yp, (present & allow).astype(np.uint8), k)
        assert np.array_equal(out_i.cpu().numpy().view(np.uint32), ei), f"P={P}/filtered/{name}: index list differs from the order-matched oracle"
        assert np.array_equal(bits(out_v.cpu().numpy()), bits(ev)), f"P={P}/filtered/{name}: scores are not bit-identical"

    # facet counts per label row % 37
    labels = np.arange(rows) % 37
    for name in ("rank1000", "zero"):
        fc, fbi, fbv, total = eng.run_facets(thr[name], vec=x, groups=labels)
        ec, ebi, ebv, et = pkg.facet_counts(yp, present, labels, 37, thr[name])
        assert total == et and np.array_equal(fc, ec) and np.array_equal(fbi, ebi) and np.array_equal(bits(fbv), bits(ebv)), f"P={P}/facets/{name}"

    # grouped top-k: groups of 7 consecutive rows
    groups = np.arange(rows) // 7
    gval, gidx, ggrp = eng.run_grouped(vec=x, groups=groups)
    ei, ev, eg, en = pkg.collapse_topk(yp, present, groups, k)
    assert gidx.size == en == k and np.array_equal(gidx, ei[:en]) and np.array_equal(bits(gval), bits(ev[:en])) and np.array_equal(ggrp, eg[:en]), f"P={P}/grouped"

    # search-after: three pages
    cursor = None
    for page in range(3):
        got = eng.run_after(cursor, vec=x)
        want = pkg.page_after(yp, present, k, cursor)
        assert (got[2], got[3], got[4]) == (want[2], want[3], want[4]), (f"P={P}/after/page {page}", got[2:], want[2:])
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), f"P={P}/after/page {page}"
        cursor = got[4]
    assert cursor[2] == pkg.CURSOR_AFTER

    # a term predicate of three clauses
    clauses, pred = pkg.bool_query(m.cols, must=[range(0, 256)], should=[range(256, 512)], must_not=[range(1000, 1024)], min_should=1)
    words, count = eng.match(clauses, pred)
    ok = pkg.match_rows(m.row, m.col, rows, clauses, pred)
    assert 0 < int(ok.sum()) < int(present.sum())
    assert count == int(ok.sum()) and np.array_equal(words, pkg.row_mask(rows, ok)), f"P={P}/match"

    # the row lookup: 64 random rows and the first and last row of every partition
    _, _, pkt_row, part_first, _ = raw
    firsts = pkt_row[part_first].astype(np.int64)
    assert firsts.size == P and firsts[0] == 0
    lasts = np.concatenate([firsts[1:] - 1, [int(np.flatnonzero(present)[-1]), rows - 1]])
    ids = np.concatenate([np.random.default_rng(P).choice(rows, 64, replace=False), firsts, lasts]).astype(np.uint32)
    sc = eng.score_rows(ids, x)
    assert np.array_equal(bits(sc[0]), bits(yp[ids])), f"P={P}/score_rows"
    rx, rl = eng.row_vectors(ids)
    for i, r in enumerate(ids):
        sel = m.row == r
        want = np.zeros(m.cols, dtype=np.float32)
        np.add.at(want, m.col[sel], m.val[sel])
        assert rl[i] == np.count_nonzero(sel) and np.array_equal(bits(rx[i]), bits(want)), f"P={P}/row_vectors/row {r}"

    print(f"\n[P={P}: {FIRST[P]} packets per partition, k={k}] tkspmv_run served by {served}; grid {info['grid']} x {info['block']}, n_groups {info['n_groups']}, "
          f"batch_mode {info['batch_mode']:#x}; after the run {_some(c1)}; after the batch of 5 {_some(c2)}; at the end {_some(eng.debug_counters())}")
    eng.close()


# ---- 4. other value types at 65 packets per partition ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision,width", [("Q1_7", 0), ("Q1_7_WIDE", 0), ("F16", 0), ("FIXED", 20), ("FIXED", 26), ("FIXED", 32)],
                         ids=["q1_7", "q1_7_wide", "f16", "fixed20", "fixed26", "fixed32"])
def test_other_value_types_at_65_packets_per_partition(pkg, oracle, second, precision, width):
    """65 packets per partition in the integer and half streams: tkspmv_run and a batch of 8, bit for bit against the value type's
    model -- the Q1.7 and W-bit integer models from the COO, the order-matched oracle over the packed half stream. TKSPMV_LOCAL is
    not forced here, so these engines stream with the device-wide exchange (stream_kernel, batch_kernel<LOCAL = false>), which never
    keeps row bases in lanes: what this covers is a partition of more than 64 packets in those streams (the request pipeline, the
    scalar row-base load), NOT the `np <= 64` branch itself -- that is test_boundary_local_thresholds' business, fp32 only."""
    k = 100
    m = second.m
    xs = second.xs if precision != "FIXED" else (second.xs * np.float32(25.0)).astype(np.float32)  # (larger scores: some sums wrap at 2.0)
    stream = pkg.Q1_7 if precision == "Q1_7_WIDE" else getattr(pkg, precision)  # (the wide variant reads the Q1.7 stream)
    packed = _pack(pkg, m, 48, SECOND, k, precision=stream, fixed_width=width)
    eng, info = _prepacked(pkg, packed, k, precision=getattr(pkg, precision))
    assert info["precision"] == getattr(pkg, precision) and info["fixed_width"] == width
    raw = packed.raw()

    def model(x):
        if precision == "Q1_7":
            return oracle.q17_scores(m.row, m.col, m.val, x, m.rows)
        if precision == "Q1_7_WIDE":
            return oracle.q17_wide_scores(m.row, m.col, m.val, x, m.rows)[:2]
        if precision == "FIXED":
            return oracle.fixed_scores(m.row, m.col, m.val, x, m.rows, width)
        return oracle.packed_scores(raw, x, m.rows, 4)

    want = [oracle.select_topk(*model(xs[q]), k) for q in range(8)]
    c0 = eng.debug_counters()
    for q in range(2):
        val, idx = _run(eng, xs[q])
        assert np.array_equal(idx, want[q][0]), f"{precision}/{width}: tkspmv_run {q}: index list differs from the model"
        assert np.array_equal(bits(val), bits(want[q][1])), f"{precision}/{width}: tkspmv_run {q}: scores are not bit-identical"
    y, _ = model(xs[1])
    assert np.array_equal(bits(eng.scores()), bits(y)), f"{precision}/{width}: tkspmv_scores differs from the model"
    bi, bv = _batch_lists(eng, xs, k)
    for q in range(8):
        assert np.array_equal(bi[q], want[q][0]), f"{precision}/{width}: batch query {q}: index list differs from the model"
        assert np.array_equal(bits(bv[q]), bits(want[q][1])), f"{precision}/{width}: batch query {q}: scores are not bit-identical"
    c1 = eng.debug_counters()
    assert info["batch_mode"] & 0xFF and c1["batch_launches"] > c0["batch_launches"] and c1["single_launches"] == 0, (info, c1)
    print(f"\n[{precision} width {width}, 65 packets per partition] batch_mode {info['batch_mode']:#x}; {_some(c0)} -> {_some(c1)}")
    eng.close()


# ---- 5. the compact stream on a prepacked engine --------------------------------------------------------------------------------
def test_compact_stream_on_a_prepacked_engine(pkg, oracle, monkeypatch, first):
    """Case 1's engine of 47 partitions (66 packets each, local thresholds forced) with two stream replicas: the batch kernel reads
    the copies re-encoded at 5 bytes per entry (the generator's values share their top four bits); with TKSPMV_F32_COMPACT=0 an
    engine of the same Packed object reads the canonical stream. Both batches equal each other and the oracle bit for bit."""
    monkeypatch.setenv("TKSPMV_LOCAL", "1")
    k = 100
    m, xs = first.m, first.xs
    packed = _pack(pkg, m, 47, FIRST, k)
    raw = packed.raw()
    lists = {}
    for compact in ("1", "0"):
        monkeypatch.setenv("TKSPMV_F32_COMPACT", compact)
        eng, info = _prepacked(pkg, packed, k, stream_replicas=2)
        assert info["batch_mode"] & 0xFF and info["batch_compact"] == int(compact), info
        assert info["batch_packet_bytes"] == 1280 if compact == "1" else info["batch_packet_bytes"] > 1280, info
        lists[compact] = _batch_lists(eng, xs[:12], k)
        print(f"\n[P=47, 2 replicas, F32_COMPACT={compact}] batch_packet_bytes {info['batch_packet_bytes']}; {_some(eng.debug_counters())}")
        eng.close()
    assert np.array_equal(lists["1"][0], lists["0"][0]) and np.array_equal(bits(lists["1"][1]), bits(lists["0"][1])), "the two streams' lists differ"
    for q in range(12):
        _exact(pkg, oracle, m, None, xs[q], k, lists["1"][0][q], lists["1"][1][q], raw, info["packet_entries"] // 64)
