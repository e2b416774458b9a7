"""The compiler's resource report of col_stats_kernel (kernel_resources.txt, written by the Makefile next to the library): no spill, no
scratch, no AGPRs, and the 128 registers and 80 KiB of LDS that let two 512-thread workgroups share a CU. Only the compiler's
summary is read."""
from test_match_resources import _report


def test_col_stats_kernels_in_resource_report():
    k = _report()
    ck = {n: v for n, v in k.items() if "tkspmv16col_stats_kernel" in n}
    # fp32 only: the 12-bit column layout, plain fp32 at 1024 / 4096 / 16384 columns, 8 entries per lane; each counting or taking
    # extremes, with and without FILT
    assert len(ck) >= 20, sorted(ck)
    for n, v in ck.items():
        assert v["VGPRs Spill"] == 0, (n, v)
        assert v["SGPRs Spill"] == 0, (n, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (n, v)
        assert v["AGPRs"] == 0, (n, v)
        # 512-thread workgroups, two per CU: 16 waves per CU, 4 per SIMD, 128 registers each
        assert v["VGPRs"] <= 128, (n, v)
        # ... and half of the CU's 160 KiB of LDS each (the array of 16384 columns is 64 KiB)
        assert v["LDS Size [bytes/block]"] <= 80 * 1024, (n, v)
