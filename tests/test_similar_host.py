"""Queries by stored row without a GPU: the symbols of every layer, argument checks that come before any device call, the shared
row lookup (csrc/row_lookup.hpp) through tkspmv_packed_get_row -- every row of every fixture and of generated and hand-made
matrices, for both entries-per-lane settings and several partition counts, compared with the COO's row entry for entry, value bits
included.

The hand-made cases assert from Packed.raw() that the situation they are made for really occurs in the packed stream."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from support import coo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HINTS = (1, 7, 64, 4064)
ROW_END, SKIP = 1, 2


def test_symbols_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    lib = pkg._lib.lib()
    for sym in ("tkspmv_enqueue_row_vectors", "tkspmv_row_vectors", "tkspmv_run_similar", "tkspmv_packed_get_row"):
        assert sym in pkg._lib.EXPORTED_SYMBOLS, sym
        assert f"int {sym}(" in hdr, sym
        assert hasattr(lib, sym), sym
    for name in ("enqueue_row_vectors", "row_vectors", "similar"):
        assert callable(getattr(pkg.SpMV, name)), name
    assert callable(pkg.Packed.get_row)
    assert callable(pkg.knn_graph) and "knn_graph" in pkg.__all__


def test_null_arguments_fail_before_any_device_call(pkg):
    lib, INVALID = pkg._lib.lib(), pkg._lib.ERR_INVALID
    rows = np.array([3, 4], dtype=np.uint32)
    xs = np.full(8, -7.0, dtype=np.float32)
    ln = np.full(2, 12345, dtype=np.uint32)
    idx = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    assert lib.tkspmv_enqueue_row_vectors(None, None, 1, None, None, None) == INVALID
    assert lib.tkspmv_enqueue_row_vectors(None, C.c_void_p(64), 0, C.c_void_p(64), None, None) == INVALID
    assert lib.tkspmv_row_vectors(None, rows.ctypes.data_as(u32p), 2, xs.ctypes.data_as(f32p), ln.ctypes.data_as(u32p)) == INVALID
    assert lib.tkspmv_run_similar(None, rows.ctypes.data_as(u32p), 2, 1, idx.ctypes.data_as(u32p), xs.ctypes.data_as(f32p)) == INVALID
    assert np.all(xs == -7.0) and np.all(ln == 12345) and np.all(idx == 0xDEADBEEF)
    n = C.c_uint32(77)
    assert lib.tkspmv_packed_get_row(None, 0, None, None, 0, C.byref(n)) == INVALID
    assert n.value == 77


def test_knn_graph_checks_k_before_building(pkg):
    m = pkg.CooMatrix(rows=1, cols=1, row=np.zeros(1, np.uint32), col=np.zeros(1, np.uint32), val=np.ones(1, np.float32))
    with pytest.raises(ValueError):
        pkg.knn_graph(m, pkg.MAX_K)  # k + 1 > MAX_K
    with pytest.raises(ValueError):
        pkg.knn_graph(m, 0)


# ---- the lookup ------------------------------------------------------------------------------------------------------------
def _words(raw, C_lane):
    """Column words of the stream, [n_packets, PE] in stream-slot order, decoded here from the raw bytes (16-bit words behind the
    values; the split 12-bit plane where a packet has 5.5 bytes per entry)."""
    packets, pb, pkt_row, _, _ = raw
    PE = 64 * C_lane
    n = pkt_row.size
    pk = packets.reshape(n, pb)
    ss = np.arange(PE)
    lane, j = ss // C_lane, ss % C_lane
    slot = (j >> 2) * 256 + lane * 4 + (j & 3)
    if pb == PE * 6:
        return pk[:, PE * 4:].copy().view("<u2")[:, slot]
    assert pb == PE * 4 + PE * 3 // 2 and C_lane == 4
    plane = pk[:, PE * 4:]
    out = np.zeros((n, PE), dtype=np.uint16)
    for l in range(64):
        a_off, b_off = (l >> 1) * 12 + (l & 1) * 8, (l >> 1) * 12 + 4 + (l & 1) * 2
        A = plane[:, a_off:a_off + 4].copy().view("<u4")[:, 0]
        B = plane[:, b_off:b_off + 2].copy().view("<u2")[:, 0].astype(np.uint32)
        cols = [(A >> 2) & 1023, (A >> 12) & 1023, (A >> 22) & 1023, (B >> 2) & 1023]
        skips = [A & 1, (A >> 1) & 1, B & 1, (B >> 1) & 1]
        for jj in range(4):
            out[:, l * 4 + jj] = (cols[jj] << 2) | (skips[jj] << 1) | ((B >> (12 + jj)) & 1)
    return out


def _check_all_rows(pkg, m, packed, label):
    """Packed.get_row(r) == the COO's row r for every r: columns and value bits, in order. Returns the row lengths."""
    lib = pkg._lib.lib()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    starts = np.searchsorted(m.row, np.arange(m.rows + 1), side="left")
    cap = int(np.max(np.diff(starts))) if m.rows else 0
    col = np.zeros(max(cap, 1), dtype=np.uint32)
    val = np.zeros(max(cap, 1), dtype=np.float32)
    n = C.c_uint32()
    mcol, mbits = m.col, m.val.view(np.uint32)
    for r in range(m.rows):
        st = lib.tkspmv_packed_get_row(packed._h, r, col.ctypes.data_as(u32p), val.ctypes.data_as(f32p), cap, C.byref(n))
        assert st == 0, (label, r, st)
        a, b = int(starts[r]), int(starts[r + 1])
        assert n.value == b - a, f"{label}: row {r} has {b - a} entries, the lookup says {n.value}"
        assert np.array_equal(col[:b - a], mcol[a:b]), f"{label}: columns of row {r}"
        assert np.array_equal(val[:b - a].view(np.uint32), mbits[a:b]), f"{label}: value bits of row {r}"
    return np.diff(starts)


def _fixtures(pkg):
    out = {}
    for f in sorted(glob.glob(os.path.join(GOLD, "gold_*.npz"))):
        z = np.load(f)
        if "row" in z.files and "col" in z.files and "rows" in z.files:
            out[os.path.basename(f)] = coo(pkg, z["rows"], z["cols"], z["row"], z["col"], z["val"])
    out["small_0indexed.mtx"] = pkg.read_mtx(os.path.join(GOLD, "small_0indexed.mtx"), index_base=0, sort=True)
    out["small_1indexed.mtx"] = pkg.read_mtx(os.path.join(GOLD, "small_1indexed.mtx"), index_base=1, sort=True)
    return out


def _every_packing(pkg, m, label):
    for c_lane in (4, 8):
        for hint in HINTS:
            packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=hint)
            yield packed, c_lane, f"{label} C={c_lane} hint={hint} parts={packed.info()['n_wave_partitions']}"
            packed.close()


def test_get_row_equals_the_coo_on_every_fixture(pkg):
    fx = _fixtures(pkg)
    assert len(fx) >= 7, sorted(fx)
    for name, m in fx.items():
        for packed, _, label in _every_packing(pkg, m, name):
            _check_all_rows(pkg, m, packed, label)
            # the convenience wrapper returns the same arrays
            r = int(m.row[m.nnz // 2])
            c, v = packed.get_row(r)
            sel = m.row == r
            assert np.array_equal(c, m.col[sel]) and np.array_equal(v.view(np.uint32), m.val[sel].view(np.uint32)), label


@pytest.mark.parametrize("dist", ["uniform", "gamma"])
@pytest.mark.parametrize("cols", [300, 1024, 4096])
def test_get_row_equals_the_coo_on_generated_matrices(pkg, dist, cols):
    m = pkg.generate_matrix(2500, cols, 20, dist, 5 + cols)
    layouts = set()
    for packed, c_lane, label in _every_packing(pkg, m, f"{dist} 2500x{cols}"):
        _check_all_rows(pkg, m, packed, label)
        layouts.add(packed.raw()[1] * 2 // (64 * c_lane))  # half bytes per entry
    # both fp32 layouts are met: 6 bytes per entry (16-bit column words) and, at C = 4 up to 1024 columns, 5.5 (12-bit words)
    assert 12 in layouts and ((11 in layouts) == (cols <= 1024))
    # the generator draws columns with replacement: rows with a repeated column exist in every test matrix
    key = m.row.astype(np.uint64) * np.uint64(1 << 20) + m.col.astype(np.uint64)
    assert np.unique(key).size < key.size


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


@pytest.mark.parametrize("cols", [1024, 4096])
def test_hand_made_rows(pkg, cols):
    m, lens = _hand_made(pkg, cols)
    for packed, c_lane, label in _every_packing(pkg, m, f"hand-made x{cols}"):
        got = _check_all_rows(pkg, m, packed, label)
        assert [int(got[r]) for r in (0, 1, 4, 9, 12, 13, 14)] == [0] * 7 and int(got[3]) == 256 and int(got[5]) == 512 and int(got[6]) == 1500
        raw = packed.raw()
        w, pkt_row = _words(raw, c_lane), raw[2]
        PE = 64 * c_lane
        # the empty rows inside [0, last stored row] are placeholders in the stream; the trailing ones have no packet at all
        assert int(np.count_nonzero(w & SKIP)) == 4 and int(pkt_row.max()) <= 11
        # the 1500-entry row spans three or more packets, the ones in the middle whole (no row end in them)
        mine = np.flatnonzero(pkt_row == 6)
        assert mine.size >= 2 and 1500 > 2 * PE
        whole = [p for p in mine if not np.any(w[p] & ROW_END)]
        assert len(whole) >= 1, label
        # (two packets that start with row 6 hold at most 2 PE - 1 < 1500 of its entries when it ends in the second: it began before)
        assert mine.size >= 3 or not np.any(w[mine[0]] & ROW_END), label


def test_partition_tails(pkg):
    """A row that ends on the last slot of a partition's last packet, and the row right behind a padded partition tail."""
    # 128 rows of 8 entries: 1024 entries, four full packets at C = 4, two at C = 8
    rows, per = 128, 8
    rng = np.random.default_rng(7)
    m = coo(pkg, rows, 512, np.repeat(np.arange(rows), per), rng.integers(0, 512, rows * per), rng.standard_normal(rows * per))
    seen_full_tail = 0
    for c_lane in (4, 8):
        PE = 64 * c_lane
        for hint in (1, 2, 4):
            packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=hint)
            label = f"exact fit C={c_lane} hint={hint}"
            _check_all_rows(pkg, m, packed, label)
            raw = packed.raw()
            w, pf, pc = _words(raw, c_lane), raw[3], raw[4]
            for q in range(pf.size):
                last = int(pf[q] + pc[q] - 1)
                if w[last, PE - 1] & ROW_END:
                    seen_full_tail += 1
            packed.close()
    assert seen_full_tail >= 6, "no partition ended on the last slot of its last packet: the case shows nothing"
    # padded tails: rows of 7 entries never fill a packet exactly; many partitions
    rows, per = 600, 7
    m = coo(pkg, rows, 300, np.repeat(np.arange(rows), per), rng.integers(0, 300, rows * per), rng.standard_normal(rows * per))
    for c_lane in (4, 8):
        PE = 64 * c_lane
        packed = pkg.Packed(m, k=8, nnz_per_lane=c_lane, n_wave_partitions=64)
        raw = packed.raw()
        w, pkt_row, pf, pc = _words(raw, c_lane), raw[2], raw[3], raw[4]
        assert pf.size >= 4
        behind_padding = []
        for q in range(pf.size - 1):
            last = int(pf[q] + pc[q] - 1)
            ends = np.flatnonzero(w[last] & ROW_END)
            if ends.size and ends[-1] < PE - 1:
                assert not np.any(w[last, ends[-1] + 1:]), "the tail of a partition's last packet is zero padding"
                behind_padding.append(int(pkt_row[pf[q + 1]]))
        assert len(behind_padding) >= 2, "no padded partition tail: the case shows nothing"
        _check_all_rows(pkg, m, packed, f"padded tails C={c_lane}")
        for r in behind_padding:  # (named: these are the rows that would start in the padding if the partition rule were missing)
            c, v = packed.get_row(r)
            assert np.array_equal(c, m.col[r * per:(r + 1) * per]) and np.array_equal(v.view(np.uint32), m.val[r * per:(r + 1) * per].view(np.uint32))
        packed.close()


def test_get_row_errors(pkg):
    lib = pkg._lib.lib()
    m = pkg.generate_matrix(200, 64, 5, "uniform", 3)
    n = C.c_uint32(0)
    packed = pkg.Packed(m, k=8)
    assert lib.tkspmv_packed_get_row(packed._h, m.rows, None, None, 0, C.byref(n)) == pkg._lib.ERR_INVALID
    assert lib.tkspmv_packed_get_row(packed._h, 0xFFFFFFFF, None, None, 0, C.byref(n)) == pkg._lib.ERR_INVALID
    assert lib.tkspmv_packed_get_row(packed._h, 0, None, None, 0, C.byref(n)) == 0  # the length alone
    assert n.value == int(np.count_nonzero(m.row == 0))
    with pytest.raises(pkg.TkspmvError) as e:
        packed.get_row(m.rows)
    assert e.value.status == pkg._lib.ERR_INVALID
    for prec in (pkg.Q1_7, pkg.F16, pkg.Q1_7_F32, pkg.FIXED):
        p = pkg.Packed(m, k=8, precision=prec)
        assert lib.tkspmv_packed_get_row(p._h, 0, None, None, 0, C.byref(n)) == pkg._lib.ERR_UNSUPPORTED, prec
        with pytest.raises(pkg.TkspmvError) as e:
            p.get_row(0)
        assert e.value.status == pkg._lib.ERR_UNSUPPORTED
        p.close()


def test_get_row_of_a_loaded_file(pkg, tmp_path):
    m = pkg.generate_matrix(1500, 1024, 20, "gamma", 9)
    packed = pkg.Packed(m, k=8, n_wave_partitions=64)
    path = tmp_path / "m.tkspmv"
    packed.save(path)
    loaded = pkg.Packed.load(path)
    _check_all_rows(pkg, m, loaded, "loaded file")
