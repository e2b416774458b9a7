"""What the compiler made of assign_kernel (the resource report the Makefile writes next to the library): which instantiations exist
and what they may use. 512-thread workgroups, two per CU: 16 waves per CU, 4 per SIMD, 128 registers each and half of the CU's
160 KiB of LDS each; the carries and running pairs of up to 16 vectors per pass stay in registers."""
import re

from support import resource_report
from test_kernel_resources import CLEAN, FAMILY_SUBSTRINGS, KIB, LDS


def _mine():
    return {n: v for n, v in resource_report().items() if "assign_kernel" in n}


def test_exactly_the_five_fp32_stream_formats():
    """The formats range_kernel has without FILT: the 12-bit column layout (QM 7) and plain fp32 (QM 0) at 1024 / 4096 / 16384 columns
    at 4 entries per lane, and 8 entries per lane at 1024 columns."""
    found = sorted(re.search(r"assign_kernelILi(\d+)ELi(\d+)ELi(\d+)E", n).groups() for n in _mine())
    assert found == sorted([("4", "1024", "7"), ("4", "1024", "0"), ("4", "4096", "0"), ("4", "16384", "0"), ("8", "1024", "0")]), found


def test_no_spill_no_scratch_and_two_workgroups_per_cu():
    mine = _mine()
    assert len(mine) == 5, sorted(mine)
    for n, v in mine.items():
        for field, value in CLEAN.items():  # no spill, no scratch, no AGPRs
            assert v[field] == value, (n, field, v)
        assert v["VGPRs"] <= 128, (n, v)
        assert v[LDS] <= 80 * KIB, (n, v)


def test_the_name_matches_no_other_family():
    for n in _mine():
        assert not any(s in n for s in FAMILY_SUBSTRINGS), n
        assert not any(s in n for s in ("row_stats_kernel", "score_rows_kernel", "col_stats_kernel")), n
