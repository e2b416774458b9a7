"""What the compiler made of nearest_kernel and nearest_fill_kernel (the resource report the Makefile writes next to the library):
which instantiations exist and what they may use. 512-thread workgroups, two per CU wherever the lists fit: 16 waves per CU, 4 per
SIMD, 128 registers each and half of the CU's 160 KiB of LDS each. The lists of 8 slots x 4 entries do not fit beside the
8-entries-per-lane scan: that instantiation is built for one workgroup per CU."""
import re

from support import resource_report
from test_kernel_resources import CLEAN, FAMILY_SUBSTRINGS, KIB, LDS

FORMATS = [("4", "1024", "7"), ("4", "1024", "0"), ("4", "4096", "0"), ("4", "16384", "0"), ("8", "1024", "0")]
ONE_WORKGROUP_PER_CU = {("8", "1024", "0", "4")}  # (C, XCOLS, QM, N): more than 128 registers, at most 256


def _mine():
    return {n: v for n, v in resource_report().items() if "nearest_kernel" in n}


def _key(name):
    return re.search(r"nearest_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups()


def test_the_five_fp32_stream_formats_with_lists_of_1_2_and_4():
    """assign_kernel's formats -- the 12-bit column layout (QM 7) and plain fp32 (QM 0) at 1024 / 4096 / 16384 columns at 4 entries
    per lane, and 8 entries per lane at 1024 columns --, each with lists of N = 1, 2 and 4 entries; and the one fill kernel."""
    found = sorted(_key(n) for n in _mine())
    assert found == sorted(f + (n,) for f in FORMATS for n in ("1", "2", "4")), found
    assert len([n for n in resource_report() if "nearest_fill_kernel" in n]) == 1


def test_no_spill_no_scratch_no_agprs():
    mine = _mine()
    assert len(mine) == 15, sorted(mine)
    fill = {n: v for n, v in resource_report().items() if "nearest_fill_kernel" in n}
    for n, v in {**mine, **fill}.items():
        for field, value in CLEAN.items():  # no spill, no scratch, no AGPRs
            assert v[field] == value, (n, field, v)
        assert v[LDS] <= 80 * KIB, (n, v)


def test_two_workgroups_per_cu_but_for_the_named_instantiation():
    for n, v in _mine().items():
        if _key(n) in ONE_WORKGROUP_PER_CU:
            assert 128 < v["VGPRs"] <= 256, (n, v)  # (were it to fit 128, it would not belong in the list)
        else:
            assert v["VGPRs"] <= 128, (n, v)


def test_the_names_match_no_other_family():
    names = [n for n in resource_report() if "nearest_kernel" in n or "nearest_fill_kernel" in n]
    assert len(names) == 16
    for n in names:
        assert not any(s in n for s in FAMILY_SUBSTRINGS), n
        assert not any(s in n for s in ("assign_kernel", "label_sums_kernel", "label_sums_close_kernel", "col_stats_kernel", "col_stats_close_kernel")), n
