"""The argument checks of the whole-matrix calls (tkspmv_enqueue_row_vectors ... tkspmv_set_boost_cosine) on the MI355X: the status
of every entry, the entry's name or the scope's prefix in its message, and -- from calls that break two rules at once -- the order
of the checks.

  every pair                                            INVALID (arguments) before UNSUPPORTED
  enqueue_score_rows, score_rows                        ... "xs = NULL: count must be 1" among the former, STATE (no query) behind
  enqueue_assign                                        ... then INVALID for dev_best = NULL with more than one pass of vectors
  enqueue_nearest, nearest                              ... UNSUPPORTED: the row scope, then the mask's; nearest: then STATE
  enqueue_col_stats, col_stats                          ... col_stats: then STATE
  enqueue_label_sums, label_sums                        ... then INVALID for "no labels given and none installed"
  enqueue_sums_close                                    INVALID only: it reads no matrix and has no scope
  sums_exponent, set_boost_cosine                       the scope of label sums / of row statistics

Only host checks run: every call here fails before anything is launched, so the engines are tiny (64 rows x 32 columns, k = 4)."""
import ctypes as C

import numpy as np
import pytest

from support import status_of

pytestmark = pytest.mark.gpu

ROWS, COLS, PER_ROW, K = 64, 32, 5, 4
ROW_SCOPE, STATS, ASSIGN, SUMS = "row vectors need", "row statistics share the row vectors' scope: ", "assignment shares the row vectors' scope: ", "label sums share the row vectors' scope: "
MASKED, COLUMNS, NO_MASK = "assignment under an allow-mask: ", "column statistics: ", "use_filter without an installed allow-mask"


@pytest.fixture(scope="module")
def engines(pkg):
    """fp32: serves every call; no query vector, no mask and no labels installed. f16: outside the stored rows' scope, which all of
    these calls share. parts: the approximate per-partition path (k > k_per_partition), inside it but outside the filtered scope."""
    rng = np.random.default_rng(7)
    row = np.repeat(np.arange(ROWS, dtype=np.uint32), PER_ROW)
    col = np.concatenate([np.sort(rng.choice(COLS, PER_ROW, replace=False)) for _ in range(ROWS)]).astype(np.uint32)
    val = rng.uniform(0.1, 1.0, row.size).astype(np.float32)
    make = lambda **kw: pkg.SpMV(row, col, val, ROWS, COLS, k=K, device=0, **kw)
    e = dict(fp32=make(), f16=make(precision=pkg.F16), parts=make(partitions=4, k_per_partition=2))
    yield e
    for eng in e.values():
        eng.close()


@pytest.fixture(scope="module")
def dev():
    """A device buffer for every pointer argument that must not be NULL (nothing is ever written: the calls fail first)."""
    import torch
    t = torch.zeros((4096,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def fails(pkg):
    """fails(status, text, entry, engine, *args): tkspmv_<entry> returns that status and its message holds the text."""
    L = pkg._lib

    def fails(status, text, entry, eng, *a):
        got = status_of(pkg, lambda: L.check(getattr(L.lib(), "tkspmv_" + entry)(eng._h, *a)))
        msg = L.lib().tkspmv_last_error().decode()
        assert got == status and text in msg, f"{entry}{a}: status {got}, expected {status}; {text!r} expected in {msg!r}"

    return fails


def _bad(entry):
    return f"bad arguments to {entry} ("


def test_stored_row_calls(pkg, engines, dev, fails):
    L, P = pkg._lib, dev.data_ptr()
    INVALID, UNSUPPORTED, STATE = L.ERR_INVALID, L.ERR_UNSUPPORTED, L.ERR_STATE
    ids, xs, out = np.zeros(4, dtype=np.uint32), np.zeros((2, COLS), dtype=np.float32), np.zeros(2 * COLS, dtype=np.float32)
    HI, HX, HO = L.u32p(ids), L.f32p(xs), L.f32p(out)
    f16, fp32 = engines["f16"], engines["fp32"]
    # row vectors: the scope's own text, no prefix
    fails(INVALID, _bad("enqueue_row_vectors"), "enqueue_row_vectors", f16, P, 0, P, None, None)
    fails(INVALID, _bad("enqueue_row_vectors"), "enqueue_row_vectors", f16, None, 1, P, None, None)
    fails(UNSUPPORTED, ROW_SCOPE, "enqueue_row_vectors", f16, P, 1, P, None, None)
    fails(INVALID, _bad("row_vectors"), "row_vectors", f16, HI, 0, HX, None)
    fails(INVALID, _bad("row_vectors"), "row_vectors", f16, HI, 1, None, None)
    fails(UNSUPPORTED, ROW_SCOPE, "row_vectors", f16, HI, 1, HX, None)
    # score_rows: both INVALID checks, the scope, then the missing query vector
    fails(INVALID, _bad("enqueue_score_rows"), "enqueue_score_rows", f16, P, 0, P, 4, 0, P, None)
    fails(INVALID, _bad("enqueue_score_rows"), "enqueue_score_rows", f16, P, 2, P, 4, 3, P, None)
    fails(INVALID, "dev_xs = NULL takes the installed query vector", "enqueue_score_rows", f16, None, 2, P, 4, 0, P, None)
    fails(UNSUPPORTED, ROW_SCOPE, "enqueue_score_rows", f16, None, 1, P, 4, 0, P, None)
    fails(STATE, "no query vector installed", "enqueue_score_rows", fp32, None, 1, P, 4, 0, P, None)
    fails(INVALID, _bad("score_rows"), "score_rows", f16, HX, 0, HI, 4, 0, HO)
    fails(INVALID, _bad("score_rows"), "score_rows", f16, HX, 2, HI, 4, 3, HO)
    fails(INVALID, "host_xs = NULL takes the installed query vector", "score_rows", f16, None, 2, HI, 4, 0, HO)
    fails(UNSUPPORTED, ROW_SCOPE, "score_rows", f16, None, 1, HI, 4, 0, HO)
    fails(STATE, "no query vector installed", "score_rows", fp32, None, 1, HI, 4, 0, HO)


def test_row_and_column_statistics(pkg, engines, dev, fails):
    L, P = pkg._lib, dev.data_ptr()
    INVALID, UNSUPPORTED, STATE = L.ERR_INVALID, L.ERR_UNSUPPORTED, L.ERR_STATE
    out = np.zeros(max(ROWS, COLS), dtype=np.float32)
    HO, HV = L.f32p(out), L.ptr(out.ctypes.data)
    f16, parts, fp32 = engines["f16"], engines["parts"], engines["fp32"]
    for kind in (-1, 4):
        fails(INVALID, _bad("enqueue_row_stats"), "enqueue_row_stats", f16, kind, P, None)
        fails(INVALID, _bad("row_stats"), "row_stats", f16, kind, HO)
    fails(INVALID, _bad("enqueue_row_stats"), "enqueue_row_stats", f16, L.ROW_NNZ, None, None)
    fails(INVALID, _bad("row_stats"), "row_stats", f16, L.ROW_NNZ, None)
    fails(UNSUPPORTED, STATS + ROW_SCOPE, "enqueue_row_stats", f16, L.ROW_L1, P, None)
    fails(UNSUPPORTED, STATS + ROW_SCOPE, "row_stats", f16, L.ROW_L1, HO)
    fails(UNSUPPORTED, STATS + ROW_SCOPE, "set_boost_cosine", f16)
    # column statistics: arguments, then the scope (the stored rows'; with a mask the filtered queries' too), then the installed mask
    for a in ((3, 1, None, 0, P, 0), (0, 0, P, 0, P, 0), (0, 2, None, 0, P, COLS), (0, 2, P, 0, P, COLS - 1), (0, 1, P, -1, P, 0), (0, 1, None, 0, None, 0)):
        fails(INVALID, _bad("enqueue_col_stats"), "enqueue_col_stats", f16, *a, None)
    fails(INVALID, _bad("enqueue_col_stats"), "enqueue_col_stats", parts, 3, 1, P, 0, P, 0, None)
    fails(UNSUPPORTED, COLUMNS + ROW_SCOPE, "enqueue_col_stats", f16, L.COL_NNZ, 1, P, 0, P, 0, None)
    fails(UNSUPPORTED, COLUMNS, "enqueue_col_stats", parts, L.COL_NNZ, 1, P, 0, P, 0, None)
    for eng in (f16, parts, fp32):
        fails(INVALID, _bad("col_stats"), "col_stats", eng, 3, 1, HV)
        fails(INVALID, _bad("col_stats"), "col_stats", eng, L.COL_MAX, 1, None)
    fails(UNSUPPORTED, COLUMNS + ROW_SCOPE, "col_stats", f16, L.COL_MAX, 1, HV)
    fails(UNSUPPORTED, COLUMNS, "col_stats", parts, L.COL_MAX, 1, HV)
    fails(STATE, NO_MASK, "col_stats", fp32, L.COL_MAX, 1, HV)


def test_assignment(pkg, engines, dev, fails):
    L, P = pkg._lib, dev.data_ptr()
    INVALID, UNSUPPORTED, STATE = L.ERR_INVALID, L.ERR_UNSUPPORTED, L.ERR_STATE
    xs, lab = np.zeros((2, COLS), dtype=np.float32), np.zeros(ROWS * 4, dtype=np.uint32)
    HX, HL = L.f32p(xs), L.u32p(lab)
    f16, parts, fp32 = engines["f16"], engines["parts"], engines["fp32"]
    for a in ((P, 0, P, P), (None, 1, P, P), (P, 1, None, P)):
        fails(INVALID, _bad("enqueue_assign"), "enqueue_assign", f16, *a, None)
    fails(UNSUPPORTED, ASSIGN + ROW_SCOPE, "enqueue_assign", f16, P, 1, P, P, None)
    # dev_best = NULL with 17 vectors, one more than a pass at this column tier: the scope comes first, then the late INVALID
    fails(UNSUPPORTED, ASSIGN + ROW_SCOPE, "enqueue_assign", f16, P, 17, P, None, None)
    fails(INVALID, "dev_best = NULL takes one pass", "enqueue_assign", fp32, P, 17, P, None, None)
    for a in ((HX, 0, HL, None), (None, 1, HL, None), (HX, 1, None, None)):
        fails(INVALID, _bad("assign"), "assign", f16, *a)
    fails(UNSUPPORTED, ASSIGN + ROW_SCOPE, "assign", f16, HX, 1, HL, None)
    # nearest: arguments; the row scope, then the mask's; the host form then asks for the installed mask
    for a in ((P, 0, 2, P, P, P), (P, 1, 0, P, P, P), (P, 1, 5, P, P, P), (None, 1, 2, P, P, P), (P, 1, 2, P, None, P)):
        fails(INVALID, _bad("enqueue_nearest"), "enqueue_nearest", f16, *a, None)
    fails(INVALID, "vectors, labels and scores given", "enqueue_nearest", parts, P, 1, 2, P, P, None, None)  # (the host form takes no scores)
    fails(UNSUPPORTED, ASSIGN + ROW_SCOPE, "enqueue_nearest", f16, P, 1, 2, P, P, P, None)
    fails(UNSUPPORTED, MASKED, "enqueue_nearest", parts, P, 1, 2, P, P, P, None)
    for a in ((HX, 0, 2, 1, HL, None), (HX, 1, 0, 1, HL, None), (HX, 1, 5, 1, HL, None), (None, 1, 2, 1, HL, None), (HX, 1, 2, 1, None, None)):
        for eng in (f16, parts, fp32):
            fails(INVALID, _bad("nearest"), "nearest", eng, *a)
    fails(INVALID, "vectors and labels given", "nearest", fp32, HX, 0, 2, 0, HL, None)
    fails(UNSUPPORTED, ASSIGN + ROW_SCOPE, "nearest", f16, HX, 1, 2, 1, HL, None)
    fails(UNSUPPORTED, MASKED, "nearest", parts, HX, 1, 2, 1, HL, None)
    fails(STATE, NO_MASK, "nearest", fp32, HX, 1, 2, 1, HL, None)


def test_label_sums(pkg, engines, dev, fails):
    L, P = pkg._lib, dev.data_ptr()
    INVALID, UNSUPPORTED = L.ERR_INVALID, L.ERR_UNSUPPORTED
    lab, sums, out = np.zeros(ROWS, dtype=np.uint32), np.zeros(4 * COLS, dtype=np.int64), np.zeros(4 * COLS, dtype=np.float32)
    HL, HS, HO = L.u32p(lab), L.i64p(sums), L.f32p(out)
    f16, fp32 = engines["f16"], engines["fp32"]
    BOTH_SINKS = L.SUMS_SINK_LDS | L.SUMS_SINK_DIRECT
    # (labels, n_bins, quantum_exp, flags, sums, mode, out): sums missing and misaligned, labels without bins and bins without labels,
    # too many bins, the mode, a float mode without an output, an unknown flag, both sinks
    for a in ((P, 4, 0, 0, None, 0, None), (P, 4, 0, 0, P + 4, 0, None), (P, 0, 0, 0, P, 0, None), (None, 4, 0, 0, P, 0, None), (P, (1 << 30) + 1, 0, 0, P, 0, None),
              (P, 4, 0, 0, P, 3, P), (P, 4, 0, 0, P, L.SUMS_FLOAT, None), (P, 4, 0, 8, P, 0, None), (P, 4, 0, BOTH_SINKS, P, 0, None)):
        fails(INVALID, _bad("enqueue_label_sums"), "enqueue_label_sums", f16, *a, None)
    fails(UNSUPPORTED, SUMS + ROW_SCOPE, "enqueue_label_sums", f16, P, 4, 0, 0, P, 0, None, None)
    fails(UNSUPPORTED, SUMS + ROW_SCOPE, "enqueue_label_sums", f16, None, 0, 0, 0, P, 0, None, None)  # (the scope before the installed labels)
    fails(INVALID, "no labels given and none installed", "enqueue_label_sums", fp32, None, 0, 0, 0, P, 0, None, None)
    # the host form has neither alignment nor flags: (labels, n_bins, quantum_exp, mode, sums, out)
    for a in ((HL, 0, 0, 0, HS, None), (None, 4, 0, 0, HS, None), (HL, (1 << 30) + 1, 0, 0, HS, None), (HL, 4, 0, 3, HS, HO), (HL, 4, 0, L.SUMS_UNIT, HS, None)):
        fails(INVALID, _bad("label_sums"), "label_sums", f16, *a)
    fails(UNSUPPORTED, SUMS + ROW_SCOPE, "label_sums", f16, HL, 4, 0, 0, HS, None)
    fails(UNSUPPORTED, SUMS + ROW_SCOPE, "label_sums", f16, None, 0, 0, 0, HS, None)
    fails(INVALID, "no labels given and none installed", "label_sums", fp32, None, 0, 0, 0, HS, None)
    # the closing launch alone: (sums, n_bins, quantum_exp, mode, out); no scope -- it reads no matrix
    for a in ((None, 4, 0, L.SUMS_FLOAT, P), (P + 4, 4, 0, L.SUMS_FLOAT, P), (P, 4, 0, L.SUMS_FLOAT, None), (P, 0, 0, L.SUMS_FLOAT, P), (P, (1 << 30) + 1, 0, L.SUMS_UNIT, P),
              (P, 4, 0, L.SUMS_RAW, P)):
        for eng in (f16, fp32):
            fails(INVALID, _bad("enqueue_sums_close"), "enqueue_sums_close", eng, *a, None)
    e = C.c_int32(0)
    fails(INVALID, _bad("sums_exponent"), "sums_exponent", f16, None)
    fails(INVALID, _bad("sums_exponent"), "sums_exponent", fp32, None)
    fails(UNSUPPORTED, SUMS + ROW_SCOPE, "sums_exponent", f16, C.byref(e))
