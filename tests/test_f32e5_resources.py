"""The batch kernel's instantiations for the compact fp32 stream (QM_F32E5, csrc/wbscsr.hpp): like the other batch kernels they sit
at the register limit of two 576-thread workgroups per CU, so the same two build checks apply -- the streaming loop touches no
scratch memory (read off the ISA of the two instantiations compiled on their own), and the compiler's resource report of the
library keeps them within 80 VGPRs and 0 AGPRs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "approximate-spmv-topk_amd", "kernel_resources.txt")
NAMES = ("_ZN6tkspmv12batch_kernelILi4ELi1024ELi9ELb0ELb0E", "_ZN6tkspmv12batch_kernelILi4ELi1024ELi9ELb0ELb1E")


def test_compact_batch_kernels_stream_without_touching_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    tu = tmp_path / "tu.hip"
    tu.write_text("""#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels/common.hpp"
#include "kernels/select.hpp"
#include "kernels/packet_math.hpp"
#include "kernels/stream_kernel.hpp"
#include "kernels/local.hpp"
#include "kernels/batch_kernel.hpp"
namespace tkspmv {
template __global__ void batch_kernel<4, 1024, QM_F32E5, false, false>(const BatchArgs);
template __global__ void batch_kernel<4, 1024, QM_F32E5, false, true>(const BatchArgs);
}
""")
    asm = tmp_path / "tu.s"
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-I" + os.path.join(ROOT, "approximate-spmv-topk_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(asm), str(tu)], stderr=subprocess.DEVNULL)
    lines = asm.read_text().split("\n")
    starts = [i for i, ln in enumerate(lines) if ln.startswith(NAMES) and "@" in ln]  # (the label line: "<name>:   ; @<name>")
    assert len(starts) == 2
    for start in starts:
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        blocks, cur = [], None
        for ln in lines[start:end]:
            if re.match(r"^\.LBB\d+_\d+:", ln):
                cur = {"name": ln.split(":")[0], "scratch": 0, "request": False, "dpp": False, "max3": False, "decode": False}
                blocks.append(cur)
            elif cur is not None:
                cur["scratch"] += "scratch_" in ln
                # a packet request: the two non-temporal buffer loads (16-byte plane, 4-byte plane)
                cur["request"] = cur["request"] or (("buffer_load_dword" in ln or "global_load_dword" in ln) and " nt" in ln)
                # the fp32 scan: DPP adds with the trigger's v_max3 behind them; the decode: the funnel shifts that rebuild values and columns
                cur["dpp"] = cur["dpp"] or "v_add_f32_dpp" in ln
                cur["max3"] = cur["max3"] or "v_max3_f32" in ln
                cur["decode"] = cur["decode"] or "v_alignbit_b32" in ln
        hot = [b for b in blocks if b["request"] or (b["dpp"] and b["max3"]) or b["decode"]]
        assert len([b for b in hot if b["request"]]) >= 3 and len([b for b in hot if b["dpp"] and b["max3"]]) >= 3, "the streaming loop was not found in the ISA of " + lines[start]
        assert all(b["scratch"] == 0 for b in hot), (lines[start], [b for b in hot if b["scratch"]])


def test_compact_batch_kernels_fit_two_workgroups_per_cu():
    if not os.path.exists(REPORT):
        pytest.skip("no resource report (the library was not built by this Makefile)")
    kernels, cur = {}, None
    for ln in open(REPORT):
        m = re.match(r"\s*Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*(VGPRs|AGPRs): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    mine = {n: v for n, v in kernels.items() if n.startswith(NAMES)}
    assert len(mine) == 2, sorted(mine)
    for n, v in mine.items():
        assert v["VGPRs"] <= 80 and v["AGPRs"] == 0, (n, v)
