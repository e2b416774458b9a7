"""Scores of given rows without a GPU: the symbols of every layer, argument checks that come before any device call, and the claim
the feature rests on -- a row's score, bit for bit as every streaming path reports it, can be computed from the row's own packets
alone -- for EVERY row: Packed.score_rows (tkspmv_packed_score_rows: the shared row lookup + the kernels' reduction restated for
the host) against the order-matched oracle over the whole stream (oracle_lib.packed_scores), on the generated and hand-made
matrices of test_similar_host.py, both entries-per-lane settings and several partition counts. Values and x are signed, so the
order of the sums shows in the bits; every test asserts that it does."""
import ctypes as C
import os

import numpy as np
import pytest

from support import bits, coo, signed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINTS = (1, 7, 64, 4096)
ROW_END, SKIP = 1, 2


def _x(cols, seed):
    return np.random.default_rng(seed).standard_normal(cols).astype(np.float32)


def _sequential(m, x):
    """Plain left-to-right fp32 sums of the rows' products (what the scores would be if the order of summation did not matter)."""
    y = np.zeros(m.rows, dtype=np.float32)
    prod = (m.val * x[m.col]).astype(np.float32)
    starts = np.searchsorted(m.row, np.arange(m.rows + 1), side="left")
    for r in range(m.rows):
        acc = np.float32(0.0)
        for p in prod[starts[r]:starts[r + 1]]:
            acc = np.float32(acc + p)
        y[r] = acc
    return y


def _every_packing(pkg, m, label, hints=HINTS):
    for c_lane in (4, 8):
        for hint in hints:
            packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=hint)
            yield packed, c_lane, f"{label} C={c_lane} hint={hint} parts={packed.info()['n_wave_partitions']}"
            packed.close()


def _check_all_rows(oracle, m, packed, c_lane, x, label):
    """Packed.score_rows(x, every row) == the oracle over the whole stream, as bits; +0.0 where the oracle saw no entries."""
    got = packed.score_rows(x, np.arange(m.rows, dtype=np.uint32))
    want, present = oracle.packed_scores(packed.raw(), x, m.rows, c_lane)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{label}: {bad.size} rows differ from the full-stream scores, first {bad[:8]}: {got[bad[:8]]} != {want[bad[:8]]}"
    assert np.all(bits(got[present == 0]) == 0), f"{label}: a row without entries does not score +0.0"
    has = np.zeros(m.rows, dtype=bool)
    has[m.row] = True
    assert np.array_equal(present.astype(bool), has), label
    return got


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    lib = pkg._lib.lib()
    for sym in ("tkspmv_enqueue_score_rows", "tkspmv_score_rows", "tkspmv_packed_score_rows"):
        assert sym in pkg._lib.EXPORTED_SYMBOLS, sym
        assert f"int {sym}(" in hdr, sym
        assert hasattr(lib, sym), sym
    for name in ("enqueue_score_rows", "score_rows", "rerank"):
        assert callable(getattr(pkg.SpMV, name)), name
    assert callable(pkg.Packed.score_rows)


def test_null_arguments_fail_before_any_device_call(pkg):
    lib, INVALID = pkg._lib.lib(), pkg._lib.ERR_INVALID
    rows = np.array([3, 4], dtype=np.uint32)
    xs = np.ones(8, dtype=np.float32)
    out = np.full(4, -7.0, dtype=np.float32)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    assert lib.tkspmv_enqueue_score_rows(None, C.c_void_p(64), 1, C.c_void_p(64), 1, 0, C.c_void_p(64), None) == INVALID
    assert lib.tkspmv_score_rows(None, xs.ctypes.data_as(f32p), 1, rows.ctypes.data_as(u32p), 2, 0, out.ctypes.data_as(f32p)) == INVALID
    assert lib.tkspmv_packed_score_rows(None, xs.ctypes.data_as(f32p), rows.ctypes.data_as(u32p), 2, out.ctypes.data_as(f32p)) == INVALID
    assert np.all(out == -7.0)


@pytest.mark.parametrize("dist", ["uniform", "gamma"])
@pytest.mark.parametrize("cols", [300, 1024, 4096])
def test_every_row_of_generated_matrices(pkg, oracle, dist, cols):
    m = signed(pkg, pkg.generate_matrix(2500, cols, 20, dist, 5 + cols), cols)
    x = _x(cols, 100 + cols)
    seq = _sequential(m, x)
    layouts, order_shows = set(), 0
    for packed, c_lane, label in _every_packing(pkg, m, f"{dist} 2500x{cols}"):
        got = _check_all_rows(oracle, m, packed, c_lane, x, label)
        layouts.add(packed.raw()[1] * 2 // (64 * c_lane))  # half bytes per entry
        order_shows += int(np.count_nonzero(bits(got) != bits(seq)))
    # both fp32 layouts are met: 6 bytes per entry (16-bit column words) and, at C = 4 up to 1024 columns, 5.5 (12-bit words)
    assert 12 in layouts and ((11 in layouts) == (cols <= 1024))
    assert order_shows > 0, "every score equals the left-to-right fp32 sum of its row: the inputs show nothing about the order"


def _hand_made(pkg, cols=1024):
    """Rows: empty rows in front, in the middle and at the end; rows of exactly 256 and 512 entries; one of 1500."""
    rng = np.random.default_rng(42)
    lens = {2: 5, 3: 256, 5: 512, 6: 1500, 7: 3, 8: 1, 10: 40, 11: 17}  # rows 0, 1, 4, 9 and 12..14 are empty
    rows = 15
    row, col, val = [], [], []
    for r in sorted(lens):
        row.append(np.full(lens[r], r, np.uint32))
        col.append(rng.integers(0, cols, lens[r]).astype(np.uint32))
        val.append(rng.standard_normal(lens[r]).astype(np.float32))
    return coo(pkg, rows, cols, np.concatenate(row), np.concatenate(col), np.concatenate(val)), lens


def _words(raw, c_lane):
    """ROW_END / SKIP flags of the stream, [n_packets, PE] in stream-slot order, decoded here from the raw bytes."""
    packets, pb, pkt_row, _, _ = raw
    PE = 64 * c_lane
    n = pkt_row.size
    pk = packets.reshape(n, pb)
    ss = np.arange(PE)
    lane, j = ss // c_lane, ss % c_lane
    slot = (j >> 2) * 256 + lane * 4 + (j & 3)
    if pb == PE * 6:
        return pk[:, PE * 4:].copy().view("<u2")[:, slot] & 3
    assert pb == PE * 4 + PE * 3 // 2 and c_lane == 4
    plane = pk[:, PE * 4:]
    out = np.zeros((n, PE), dtype=np.uint16)
    for l in range(64):
        a_off, b_off = (l >> 1) * 12 + (l & 1) * 8, (l >> 1) * 12 + 4 + (l & 1) * 2
        A = plane[:, a_off:a_off + 4].copy().view("<u4")[:, 0]
        B = plane[:, b_off:b_off + 2].copy().view("<u2")[:, 0].astype(np.uint32)
        skips = [A & 1, (A >> 1) & 1, B & 1, (B >> 1) & 1]
        for jj in range(4):
            out[:, l * 4 + jj] = (skips[jj] << 1) | ((B >> (12 + jj)) & 1)
    return out


@pytest.mark.parametrize("cols", [1024, 4096])
def test_hand_made_rows(pkg, oracle, cols):
    m, lens = _hand_made(pkg, cols)
    x = _x(cols, 7)
    seq = _sequential(m, x)
    for packed, c_lane, label in _every_packing(pkg, m, f"hand-made x{cols}"):
        got = _check_all_rows(oracle, m, packed, c_lane, x, label)
        raw = packed.raw()
        w, pkt_row = _words(raw, c_lane), raw[2]
        # the empty rows inside [0, last stored row] are placeholders in the stream; the trailing ones have no packet at all
        assert int(np.count_nonzero(w & SKIP)) == 4 and int(pkt_row.max()) <= 11, label
        assert np.all(bits(got[[0, 1, 4, 9, 12, 13, 14]]) == 0), label
        # the 1500-entry row spans three or more packets, one in the middle whole (no row end in it)
        mine = np.flatnonzero(pkt_row == 6)
        assert any(not np.any(w[p] & ROW_END) for p in mine), label
        # the long rows' sums are not the left-to-right ones: the wave's order of summation is what was compared
        assert bits(got[6]) != bits(seq[6]) or bits(got[5]) != bits(seq[5]) or bits(got[3]) != bits(seq[3]), label
        # any order of the ids, repeated ids
        ids = np.array([6, 0, 14, 6, 3, 8, 5, 5, 2], dtype=np.uint32)
        assert np.array_equal(bits(packed.score_rows(x, ids)), bits(got[ids])), label


def test_partition_tails(pkg, oracle):
    """Rows that end on the last slot of a partition's last packet, and the rows right behind a padded partition tail."""
    rows, per = 128, 8  # 1024 entries: four full packets at C = 4, two at C = 8
    rng = np.random.default_rng(7)
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    x = _x(512, 8)
    seen_full_tail = 0
    for packed, c_lane, label in _every_packing(pkg, m, "exact fit", hints=(1, 2, 4)):
        _check_all_rows(oracle, m, packed, c_lane, x, label)
        raw = packed.raw()
        w, pf, pc = _words(raw, c_lane), raw[3], raw[4]
        seen_full_tail += sum(1 for q in range(pf.size) if w[int(pf[q] + pc[q] - 1), 64 * c_lane - 1] & ROW_END)
    assert seen_full_tail >= 6, "no partition ended on the last slot of its last packet: the case shows nothing"
    rows, per = 600, 7  # rows of 7 entries never fill a packet exactly; many partitions
    m = coo(pkg, rows, 300, np.repeat(np.arange(rows), per), rng.integers(0, 300, rows * per), rng.standard_normal(rows * per))
    x = _x(300, 9)
    for packed, c_lane, label in _every_packing(pkg, m, "padded tails", hints=(64,)):
        PE = 64 * c_lane
        raw = packed.raw()
        w, pf, pc = _words(raw, c_lane), raw[3], raw[4]
        padded = 0
        for q in range(pf.size - 1):
            ends = np.flatnonzero(w[int(pf[q] + pc[q] - 1)] & ROW_END)
            padded += int(ends.size and ends[-1] < PE - 1)
        assert pf.size >= 4 and padded >= 2, "no padded partition tail: the case shows nothing"
        _check_all_rows(oracle, m, packed, c_lane, x, label)


def test_rows_of_a_loaded_file(pkg, oracle, tmp_path):
    m = signed(pkg, pkg.generate_matrix(1500, 1024, 20, "gamma", 9), 9)
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    path = tmp_path / "m.tkspmv"
    packed.save(path)
    loaded = pkg.Packed.load(path)
    x = _x(1024, 10)
    got = _check_all_rows(oracle, m, loaded, 4, x, "loaded file")
    assert np.array_equal(bits(got), bits(packed.score_rows(x, np.arange(m.rows))))
    assert np.count_nonzero(bits(got) != bits(_sequential(m, x))) > 0


def test_errors(pkg):
    lib = pkg._lib.lib()
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    x = _x(64, 1)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    packed = pkg.Packed(m, k=8)

    def call(p, rows, n=None, out=None):
        rows = np.asarray(rows, dtype=np.uint32)
        out = np.full(max(rows.size, 1), -7.0, dtype=np.float32) if out is None else out
        return lib.tkspmv_packed_score_rows(p._h, x.ctypes.data_as(f32p), rows.ctypes.data_as(u32p), rows.size if n is None else n, out.ctypes.data_as(f32p)), out

    INVALID, UNSUPPORTED = pkg._lib.ERR_INVALID, pkg._lib.ERR_UNSUPPORTED
    for bad in ([m.rows], [0xFFFFFFFF], [0, 1, m.rows, 2]):
        st, out = call(packed, bad)
        assert st == INVALID and np.all(out == -7.0), bad  # (nothing is written by a rejected call)
    assert call(packed, [0], n=0)[0] == INVALID and call(packed, [0], n=-1)[0] == INVALID
    assert lib.tkspmv_packed_score_rows(packed._h, None, None, 1, None) == INVALID
    st, out = call(packed, [0, m.rows - 1])
    assert st == 0 and np.all(out != -7.0)
    with pytest.raises(pkg.TkspmvError) as e:
        packed.score_rows(x, [m.rows])
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        packed.score_rows(x[:-1], [0])
    assert packed.score_rows(x, []).shape == (0,)
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        p = pkg.Packed(m, k=8, precision=prec)
        assert call(p, [0])[0] == UNSUPPORTED, prec
        with pytest.raises(pkg.TkspmvError) as e:
            p.score_rows(x, [0])
        assert e.value.status == UNSUPPORTED
        p.close()
