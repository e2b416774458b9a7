"""The order of the argument checks of the query forms (tkspmv_enqueue_filtered ... tkspmv_enqueue_score_rows and the tkspmv_run_*
host forms) on the MI355X: a call that breaks two rules at once returns the status of the check that comes first.

  enqueue_filtered, enqueue_range                       UNSUPPORTED before INVALID
  enqueue_grouped, _after, _facets, _match,
  enqueue_row_vectors, _score_rows                      INVALID before UNSUPPORTED; "dev_xs = NULL: count must be 1" is one of them
  run_range                                             UNSUPPORTED, INVALID (arguments), INVALID (use_filter), STATE
  run_facets                                            UNSUPPORTED, INVALID (use_filter), STATE (query), STATE (labels)
  run_after                                             INVALID (use_filter), UNSUPPORTED, STATE
  run_grouped                                           INVALID (use_filter), then enqueue_grouped's own order

Only host checks run: every call here fails before anything is launched, so the engines are tiny (64 rows x 32 columns, k = 4)."""
import ctypes as C

import numpy as np
import pytest

from support import status_of

pytestmark = pytest.mark.gpu

ROWS, COLS, PER_ROW, K = 64, 32, 5, 4


@pytest.fixture(scope="module")
def engines(pkg):
    """fp32: serves every form; no query vector, no mask and no labels installed. f16: outside the filtered / range scope and the
    stored-row forms. parts: the approximate per-partition path (k > k_per_partition), outside the grouped and the filtered scope."""
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


def test_enqueue_forms_outside_their_scope(pkg, engines, dev):
    L = pkg._lib
    P = dev.data_ptr()
    for name in ("f16", "parts"):  # both outside filter_unsupported / range_unsupported
        eng = engines[name]
        assert status_of(pkg, eng.enqueue_filtered, P, 0, P) == L.ERR_UNSUPPORTED, name
        assert status_of(pkg, eng.enqueue_range, P, 0, P, P) == L.ERR_UNSUPPORTED, name
        assert status_of(pkg, eng.enqueue_facets, P, 0, P, P) == L.ERR_INVALID, name
        assert status_of(pkg, eng.enqueue_facets, 0, 2, P, P) == L.ERR_INVALID, name
    eng = engines["parts"]  # outside grouped_unsupported
    assert status_of(pkg, eng.enqueue_grouped, P, 0) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_after, P, 0) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_after, 0, 2) == L.ERR_INVALID
    eng = engines["f16"]  # outside row_vectors_unsupported / match_unsupported
    assert status_of(pkg, eng.enqueue_score_rows, 0, 2, P, 4, P) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_score_rows, P, 0, P, 4, P) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_row_vectors, P, 0, P) == L.ERR_INVALID
    assert status_of(pkg, eng.enqueue_match, P, P, 0, P) == L.ERR_INVALID
    # ... and the same calls with valid arguments say UNSUPPORTED
    assert status_of(pkg, engines["parts"].enqueue_grouped, P, 1) == L.ERR_UNSUPPORTED
    assert status_of(pkg, engines["parts"].enqueue_after, P, 1) == L.ERR_UNSUPPORTED
    assert status_of(pkg, engines["f16"].enqueue_facets, P, 1, P, P) == L.ERR_UNSUPPORTED
    assert status_of(pkg, engines["f16"].enqueue_score_rows, P, 1, P, 4, P) == L.ERR_UNSUPPORTED
    assert status_of(pkg, engines["f16"].enqueue_row_vectors, P, 1, P) == L.ERR_UNSUPPORTED
    assert status_of(pkg, engines["f16"].enqueue_match, P, P, 1, P) == L.ERR_UNSUPPORTED


def test_host_forms_outside_their_scope(pkg, engines):
    L = pkg._lib
    lib = L.lib()
    n, total, cnt, nxt = C.c_int32(0), C.c_uint32(0), C.c_uint64(0), L.Cursor()
    # run_after: use_filter without a mask comes before the scope
    assert lib.tkspmv_run_after(engines["parts"]._h, None, 1, None, None, C.byref(n), C.byref(total), C.byref(nxt)) == L.ERR_INVALID
    assert lib.tkspmv_run_after(engines["parts"]._h, None, 0, None, None, C.byref(n), C.byref(total), C.byref(nxt)) == L.ERR_UNSUPPORTED
    for name in ("f16", "parts"):
        h = engines[name]._h
        # run_range / run_facets: the scope comes before use_filter without a mask, and before bad arguments
        assert lib.tkspmv_run_range(h, 0.5, 1, None, None, 0, C.byref(cnt)) == L.ERR_UNSUPPORTED, name
        assert lib.tkspmv_run_range(h, 0.5, 1, None, None, 4, None) == L.ERR_UNSUPPORTED, name
        assert lib.tkspmv_run_facets(h, 0.5, 1, None, None, C.byref(cnt)) == L.ERR_UNSUPPORTED, name
    # run_grouped: use_filter without a mask comes before enqueue_grouped's checks (here: the scope)
    assert lib.tkspmv_run_grouped(engines["parts"]._h, 1, None, None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.tkspmv_run_grouped(engines["parts"]._h, 0, None, None, None, C.byref(n)) == L.ERR_UNSUPPORTED


def test_host_forms_without_query_mask_and_labels(pkg, engines):
    L = pkg._lib
    lib = L.lib()
    h = engines["fp32"]._h
    n, total, cnt, nxt = C.c_int32(0), C.c_uint32(0), C.c_uint64(0), L.Cursor()
    # use_filter without a mask (INVALID) comes before the missing query vector and the missing labels (STATE) ...
    assert lib.tkspmv_run_range(h, 0.5, 1, None, None, 0, C.byref(cnt)) == L.ERR_INVALID
    assert lib.tkspmv_run_facets(h, 0.5, 1, None, None, C.byref(cnt)) == L.ERR_INVALID
    assert lib.tkspmv_run_grouped(h, 1, None, None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.tkspmv_run_after(h, None, 1, None, None, C.byref(n), C.byref(total), C.byref(nxt)) == L.ERR_INVALID
    # ... bad arguments too ...
    assert lib.tkspmv_run_range(h, 0.5, 0, None, None, 4, C.byref(cnt)) == L.ERR_INVALID
    # ... and without use_filter the calls get as far as the state
    assert lib.tkspmv_run_range(h, 0.5, 0, None, None, 0, C.byref(cnt)) == L.ERR_STATE
    assert lib.tkspmv_run_facets(h, 0.5, 0, None, None, C.byref(cnt)) == L.ERR_STATE
    assert lib.tkspmv_run_grouped(h, 0, None, None, None, C.byref(n)) == L.ERR_STATE
    assert lib.tkspmv_run_after(h, None, 0, None, None, C.byref(n), C.byref(total), C.byref(nxt)) == L.ERR_STATE
