"""Filtered top-k without a GPU: the allow-mask packing of row_mask(), and the ISA of stream_filter_kernel
(the streaming loop touches no scratch and waits for no chain of single loads; the mask words travel on the scalar unit)."""
import os
import re

import numpy as np
import pytest

from support import INCLUDE, compile_device_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask_loop(rows, allow):
    words = np.zeros(max(1, (rows + 31) // 32), dtype=np.uint32)
    for r in range(rows):
        if allow[r]:
            words[r >> 5] |= np.uint32(1 << (r & 31))
    return words


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 100, 1000, 4097])
def test_row_mask_packs_lsb_first(pkg, rows):
    rng = np.random.default_rng(rows)
    allow = rng.random(rows) < 0.4
    w = pkg.row_mask(rows, allow)
    assert w.dtype == np.uint32 and w.shape == ((rows + 31) // 32,)
    assert np.array_equal(w, _mask_loop(rows, allow))
    # numpy's own little-endian bit order, as the header documents
    padded = np.zeros(w.size * 32, dtype=bool)
    padded[:rows] = allow
    assert np.array_equal(w, np.packbits(padded, bitorder="little").view("<u4"))
    # no mask: every row, and nothing beyond rows
    full = pkg.row_mask(rows)
    assert np.array_equal(full, _mask_loop(rows, np.ones(rows, dtype=bool)))


@pytest.mark.parametrize("rows", [5, 64, 77, 1000])
def test_row_mask_exclude(pkg, rows):
    rng = np.random.default_rng(7 + rows)
    ex = rng.choice(rows, size=max(1, rows // 5), replace=False)
    allow = np.ones(rows, dtype=bool)
    allow[ex] = False
    assert np.array_equal(pkg.row_mask(rows, exclude=ex), _mask_loop(rows, allow))
    base = rng.random(rows) < 0.5
    both = base.copy()
    both[ex] = False
    assert np.array_equal(pkg.row_mask(rows, base, exclude=ex), _mask_loop(rows, both))
    assert np.array_equal(pkg.row_mask(rows, exclude=[]), pkg.row_mask(rows))


def test_row_mask_rejects_bad_input(pkg):
    with pytest.raises(ValueError):
        pkg.row_mask(100, np.ones(99, dtype=bool))
    with pytest.raises(ValueError):
        pkg.row_mask(100, np.ones(101, dtype=bool))
    with pytest.raises(ValueError):
        pkg.row_mask(100, np.ones(100, dtype=np.int32))
    with pytest.raises(ValueError):
        pkg.row_mask(100, exclude=[100])
    with pytest.raises(ValueError):
        pkg.row_mask(100, exclude=[-1])


def test_filter_symbols_exported(pkg):
    assert "tkspmv_enqueue_filtered" in pkg._lib.EXPORTED_SYMBOLS and "tkspmv_set_filter" in pkg._lib.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    assert "int tkspmv_enqueue_filtered(" in hdr and "int tkspmv_set_filter(" in hdr
    for name in ("enqueue_filtered", "set_filter", "run_filtered"):
        assert callable(getattr(pkg.SpMV, name))


def _compile_filter_kernels(tmp_path):
    return compile_device_only(tmp_path, """#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels/common.hpp"
#include "kernels/select.hpp"
#include "kernels/packet_math.hpp"
#include "kernels/stream_kernel.hpp"
namespace tkspmv {
template __global__ void stream_filter_kernel<4, false, 1024, 7, 3>(const StreamParams, const SelectParams, const FilterParams);
template __global__ void stream_filter_kernel<4, false, 1024, 0, 3>(const StreamParams, const SelectParams, const FilterParams);
template __global__ void stream_filter_kernel<4, false, 16384, 0, 3>(const StreamParams, const SelectParams, const FilterParams);
template __global__ void stream_filter_kernel<8, false, 1024, 0, 2>(const StreamParams, const SelectParams, const FilterParams);
}
""", (INCLUDE,)).split("\n")


def test_filter_kernel_isa(tmp_path):
    lines = _compile_filter_kernels(tmp_path)
    starts = [i for i, ln in enumerate(lines) if ln.startswith("_ZN6tkspmv20stream_filter_kernel") and "@" in ln]
    assert len(starts) == 4
    for start in starts:
        name = lines[start].split(":")[0]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[start:end]
        # (1) the streaming blocks touch no scratch (pattern of test_kernel_resources.py)
        blocks, cur = [], None
        for ln in body:
            if re.match(r"^\.LBB\d+_\d+:", ln):
                cur = {"scratch": 0, "hot": False, "dpp": False, "max3": False}
                blocks.append(cur)
            elif cur is not None:
                cur["scratch"] += "scratch_" in ln
                if ("global_load_dword" in ln or "buffer_load_dword" in ln) and " nt" in ln:
                    cur["hot"] = True
                cur["dpp"] = cur["dpp"] or "v_add_f32_dpp" in ln
                cur["max3"] = cur["max3"] or "v_max3_f32" in ln
        hot = [b for b in blocks if b["hot"] or (b["dpp"] and b["max3"])]
        assert len(hot) >= 3, "the streaming loop was not found in the ISA of " + name
        if "stream_filter_kernelILi8E" not in name:  # (the 8-entries-per-lane variant: see the resource test above)
            assert all(b["scratch"] == 0 for b in hot), name
        # (2) no run of (wait for every load, ONE load): the chain check of test_kernel_resources.py
        seq = []
        for ln in body:
            t = ln.strip().split(";")[0].strip()
            if not ln.startswith("\t") or not t:
                continue
            if t.startswith(("global_load", "buffer_load", "flat_load")):
                seq.append("L")
            elif t.startswith("s_waitcnt") and "vmcnt(0)" in t:
                seq.append("W")
            elif t.startswith(("global_store", "global_atomic", "s_sleep")):
                seq.append("x")
        runs = [len(m.group(0)) // 2 for m in re.finditer(r"(?:WL){6,}", "".join(seq))]
        assert runs == [], (name, runs)
        # (3) the mask words are scalar loads: no flat access anywhere in the kernel (one would force vmcnt(0) in the loop)
        assert not any(ln.strip().startswith("flat_") for ln in body), name
