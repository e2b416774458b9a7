"""The compiler's resource report of match_kernel (kernel_resources.txt, written by the Makefile next to the library): no spill, no
scratch, no AGPRs, and the 128 registers and 80 KiB of LDS that let two 512-thread workgroups share a CU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "approximate-spmv-topk_amd", "kernel_resources.txt")


def _report():
    if not os.path.exists(REPORT):
        pytest.skip("no resource report (the library was not built by this Makefile)")
    kernels, cur = {}, None
    for ln in open(REPORT):
        m = re.match(r"\s*Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return kernels


def test_match_kernels_in_resource_report():
    k = _report()
    mk = {n: v for n, v in k.items() if "tkspmv12match_kernel" in n}
    # fp32 only: the 12-bit column layout, plain fp32 at 1024 / 4096 / 16384 columns, 8 entries per lane; each with and without FILT
    assert len(mk) >= 10, sorted(mk)
    for n, v in mk.items():
        assert v["VGPRs Spill"] == 0, (n, v)
        assert v["SGPRs Spill"] == 0, (n, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (n, v)
        assert v["AGPRs"] == 0, (n, v)
        # 512-thread workgroups, two per CU: 16 waves per CU, 4 per SIMD, 128 registers each
        assert v["VGPRs"] <= 128, (n, v)
        # ... and half of the CU's 160 KiB of LDS each (the table of 16384 columns is 64 KiB)
        assert v["LDS Size [bytes/block]"] <= 80 * 1024, (n, v)
