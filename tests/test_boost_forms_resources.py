"""What the compiler made of boosted_hits_kernel and boosted_bins_kernel (the resource report the Makefile writes next to the
library): each exists once and runs 256-thread workgroups at full occupancy, like boost_cut_kernel whose geometry they share. The
facet sink's histogram is LDS sized per launch (at most 4096 bins of 12 bytes): the report shows none."""
from support import resource_report
from test_kernel_resources import CLEAN, FAMILY_SUBSTRINGS, KIB, LDS

BUDGET = {
    "boosted_hits_kernel": dict(equal={**CLEAN, LDS: 0}, at_most={"VGPRs": 64}),
    "boosted_bins_kernel": dict(equal=CLEAN, at_most={"VGPRs": 64, LDS: 64 * KIB}),
}


def test_each_kernel_once_within_its_budget():
    k = resource_report()
    for name, row in BUDGET.items():
        mine = {n: v for n, v in k.items() if name in n}
        assert len(mine) == 1, (name, sorted(mine))
        for n, v in mine.items():
            for field, value in row["equal"].items():
                assert v[field] == value, (n, field, v)
            for field, limit in row["at_most"].items():
                assert v[field] <= limit, (n, field, v)


def test_the_names_match_no_other_family():
    names = [n for n in resource_report() if any(mine in n for mine in BUDGET)]
    assert len(names) == 2, names
    for n in names:
        assert not any(s in n for s in FAMILY_SUBSTRINGS + ("select_kernel",)), n
