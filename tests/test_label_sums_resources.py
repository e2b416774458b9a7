"""What the compiler made of label_sums_kernel (the resource report the Makefile writes next to the library): which instantiations exist
and what they may use. 512-thread workgroups, two per CU: 16 waves per CU, 4 per SIMD, 128 registers each and half of the CU's
160 KiB of LDS each; the LDS sink holds 64 KiB of 64-bit bins, the direct sink no LDS at all."""
import re

from support import resource_report
from test_kernel_resources import CLEAN, FAMILY_SUBSTRINGS, KIB, LDS


def _mine():
    return {n: v for n, v in resource_report().items() if "label_sums_kernel" in n}


def test_exactly_the_nine_instantiations():
    """(C, XCOLS, C12, LDS_SINK): the direct sink for the five fp32 stream formats of assign_kernel -- the 12-bit column layout and
    plain fp32 at 1024 / 4096 / 16384 columns at 4 entries per lane, 8 entries per lane at 1024 columns --, the LDS sink for the four
    of them below the 16384-column tier."""
    found = sorted(re.search(r"label_sums_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E", n).groups() for n in _mine())
    formats = [("4", "1024", "1"), ("4", "1024", "0"), ("4", "4096", "0"), ("4", "16384", "0"), ("8", "1024", "0")]
    assert found == sorted([f + ("0",) for f in formats] + [f + ("1",) for f in formats if f[1] != "16384"]), found


def test_no_spill_no_scratch_and_two_workgroups_per_cu():
    mine = _mine()
    assert len(mine) == 9, sorted(mine)
    for n, v in mine.items():
        for field, value in CLEAN.items():  # no spill, no scratch, no AGPRs
            assert v[field] == value, (n, field, v)
        assert v["VGPRs"] <= 128, (n, v)
        assert v[LDS] <= 80 * KIB, (n, v)
        assert v[LDS] == (64 * KIB if n.endswith("Lb1EEEvNS_12StreamParamsENS_15LabelSumsParamsE") else 0), (n, v)
    close = {n: v for n, v in resource_report().items() if "label_sums_close_kernel" in n}
    assert len(close) == 1
    for v in close.values():
        assert all(v[field] == value for field, value in CLEAN.items()) and v[LDS] <= 1 * KIB, v


def test_the_names_match_no_other_family():
    for n in list(_mine()) + [n for n in resource_report() if "label_sums_close_kernel" in n]:
        assert not any(s in n for s in FAMILY_SUBSTRINGS), n
        assert not any(s in n for s in ("row_stats_kernel", "score_rows_kernel", "col_stats_kernel", "assign_kernel")), n
