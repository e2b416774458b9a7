"""Range queries without a GPU: the symbols of every layer, the RANGE_PERIOD option, argument checks that come before any device
call, and the ISA of range_kernel (the streaming loop touches no scratch, waits for no chain of single loads,
makes no flat access; the mask words travel on the scalar unit)."""
import ctypes as C
import os
import re

from support import INCLUDE, compile_device_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_symbols_in_every_layer(pkg):
    assert "tkspmv_enqueue_range" in pkg._lib.EXPORTED_SYMBOLS and "tkspmv_run_range" in pkg._lib.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "tkspmv.h")).read()
    assert "int tkspmv_enqueue_range(" in hdr and "int tkspmv_run_range(" in hdr
    lib = pkg._lib.lib()
    assert hasattr(lib, "tkspmv_enqueue_range") and hasattr(lib, "tkspmv_run_range")
    for name in ("enqueue_range", "run_range"):
        assert callable(getattr(pkg.SpMV, name))
    assert callable(pkg.range_spmv) and "range_spmv" in pkg.__all__


def test_range_period_is_a_documented_option(pkg):
    opts = {o["name"]: o for o in pkg.options()}
    assert "RANGE_PERIOD" in opts
    assert opts["RANGE_PERIOD"]["kind"] == "tuning" and opts["RANGE_PERIOD"]["doc"] and opts["RANGE_PERIOD"]["values"]
    pkg.set_option("RANGE_PERIOD", 0)
    assert pkg.get_option("RANGE_PERIOD") == "0"
    pkg.set_option("RANGE_PERIOD", None)


def test_null_engine_fails_before_any_device_call(pkg):
    lib = pkg._lib.lib()
    count = C.c_uint64(7)
    assert lib.tkspmv_enqueue_range(None, None, 1, None, None, 0, None, None, 0, None, None) == pkg._lib.ERR_INVALID
    assert lib.tkspmv_run_range(None, 0.5, 0, None, None, 0, C.byref(count)) == pkg._lib.ERR_INVALID
    assert count.value == 7


def _compile_range_kernels(tmp_path):
    return compile_device_only(tmp_path, """#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels/common.hpp"
#include "kernels/select.hpp"
#include "kernels/packet_math.hpp"
#include "kernels/stream_kernel.hpp"
#include "kernels/local.hpp"
#include "kernels/batch_kernel.hpp"
#include "kernels/range_kernel.hpp"
namespace tkspmv {
template __global__ void range_kernel<4, 1024, 7, false, 3>(const StreamParams, const RangeParams);
template __global__ void range_kernel<4, 1024, 7, true, 3>(const StreamParams, const RangeParams);
template __global__ void range_kernel<4, 16384, 0, true, 3>(const StreamParams, const RangeParams);
template __global__ void range_kernel<8, 1024, 0, true, 2>(const StreamParams, const RangeParams);
}
""", (INCLUDE,)).split("\n")


def test_range_kernel_isa(tmp_path):
    lines = _compile_range_kernels(tmp_path)
    starts = [i for i, ln in enumerate(lines) if ln.startswith("_ZN6tkspmv12range_kernel") and "@" in ln]
    assert len(starts) == 4
    for start in starts:
        name = lines[start].split(":")[0]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[start:end]
        # (1) no scratch instruction in a block that requests a packet or runs the scan (pattern of test_kernel_resources.py)
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
        # (3) no flat access anywhere in the kernel (one would force vmcnt(0) in the loop)
        assert not any(ln.strip().startswith("flat_") for ln in body), name
    # (4) FILT: the mask words travel as scalar loads. The two 12-bit instantiations differ in FILT alone, and neither makes a flat
    # access (3): what the filtered one loads in addition must be the single-dword scalar loads of mask_pair / mask_rows.
    def count(tag, prefix):
        start = next(s for s in starts if tag in lines[s])
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        return sum(1 for ln in lines[start:end] if ln.strip().startswith(prefix))
    plain, filt = "Li4ELi1024ELi7ELb0E", "Li4ELi1024ELi7ELb1E"
    assert count(filt, "s_load_dword ") >= count(plain, "s_load_dword ") + 2
    assert count(filt, "global_load") == count(plain, "global_load") and count(filt, "buffer_load") == count(plain, "buffer_load")
