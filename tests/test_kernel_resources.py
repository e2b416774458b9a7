"""Build checks on what the compiler made of the kernels: its resource report (Makefile: -Rpass-analysis=kernel-resource-usage ->
approximate-spmv-topk_amd/kernel_resources.txt) and the ISA of kernels compiled on their own. BUDGET states in one table what each
kernel family is allowed; a miss is a regression no functional test sees (at 81+ registers the dispatcher
places one 576-thread workgroup per CU instead of two, and every query takes twice as long). What does not fit the table's shape --
the streaming kernels' exemptions, which instantiations exist, the ISA -- is a test function of its own below."""
import re

import pytest

from support import INCLUDE, compile_device_only, resource_report

KIB = 1024
SPILL, SGPR_SPILL, SCRATCH, LDS = "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"
CLEAN = {"AGPRs": 0, SPILL: 0, SGPR_SPILL: 0, SCRATCH: 0}  # no spill, no scratch, no AGPRs

# One row per family: the kernels whose name contains one of `names` (and none of `unless`); how many the report must hold
# (`exactly`, or `at_least`); per field the value it must have (`equal`) or may not exceed (`at_most`).
BUDGET = {
    # fp32 only: the 12-bit column layout, plain fp32 at 1024 / 4096 / 16384 columns, 8 entries per lane; each with and without
    # FILT. 512-thread workgroups, two per CU: 16 waves per CU, 4 per SIMD, 128 registers each, and half of the CU's 160 KiB of LDS
    # each. (The facet kernels' SGPR spill: test_facet_kernels_spill_no_sgprs.)
    "facet": dict(names=("tkspmv12facet_kernel",), at_least=10, equal={SPILL: 0, SCRATCH: 0, "AGPRs": 0}, at_most={"VGPRs": 128, LDS: 80 * KIB}),
    # the same instantiations and the same two workgroups per CU (the table of 16384 columns is 64 KiB)
    "match": dict(names=("tkspmv12match_kernel",), at_least=10, equal=CLEAN, at_most={"VGPRs": 128, LDS: 80 * KIB}),
    # ... each counting or taking extremes, with and without FILT (the array of 16384 columns is 64 KiB)
    "col_stats": dict(names=("tkspmv16col_stats_kernel",), at_least=20, equal=CLEAN, at_most={"VGPRs": 128, LDS: 80 * KIB}),
    # the compact fp32 stream's two batch kernels sit at the register limit of two 576-thread workgroups per CU like the others
    "batch_f32e5": dict(names=("_ZN6tkspmv12batch_kernelILi4ELi1024ELi9ELb0ELb0E", "_ZN6tkspmv12batch_kernelILi4ELi1024ELi9ELb0ELb1E"), exactly=2,
                        equal={"AGPRs": 0}, at_most={"VGPRs": 80}),
    # fp32 only: the 12-bit column layout, plain fp32 at 1024 / 4096 / 16384 columns, 8 entries per lane; each with and without SCORES
    "filter": dict(names=("tkspmv20stream_filter_kernel",), exactly=10, equal={"AGPRs": 0}),
    # (the opt-in 8-entries-per-lane top-k variant sits at the register limit and spills, like its unfiltered twin: the exemption
    #  test_streaming_kernels_do_not_spill_and_fit_two_workgroups_per_cu grants stream_kernel<8, false>)
    "filter_but_c8_topk": dict(names=("tkspmv20stream_filter_kernel",), unless=("stream_filter_kernelILi8ELb0E",), exactly=9, equal={SPILL: 0, SCRATCH: 0}),
    # the top-k variants (not SCORES): two 576-thread workgroups per CU, like stream_kernel
    "filter_topk": dict(names=("stream_filter_kernelILi4ELb0E", "stream_filter_kernelILi8ELb0E"), exactly=5, at_most={"VGPRs": 80}),
    # fp32 only, the filter kernels' layouts, each with and without FILT. 512-thread workgroups (8 streaming waves, no server wave),
    # two per CU: 16 waves per CU, 4 per SIMD, 128 registers each
    "range": dict(names=("tkspmv12range_kernel",), exactly=10, equal={"AGPRs": 0}, at_most={"VGPRs": 128}),
    "range_c4": dict(names=("range_kernelILi4E",), exactly=8, equal={SPILL: 0, SCRATCH: 0}),
    # the 12-bit column layout, plain fp32 at 1024 / 4096 / 16384 columns, 8 entries per lane
    "row_vectors": dict(names=("row_vectors_kernel",), exactly=5, equal=CLEAN),
    # the 12-bit column layout, plain fp32 at 4 entries per lane (every column tier: x is not staged in LDS), 8 entries per lane
    "score_rows": dict(names=("score_rows_kernel",), exactly=3, equal=CLEAN),
    # ... and four kinds each
    "row_stats": dict(names=("row_stats_kernel",), exactly=12, equal=CLEAN),
    # 256-thread workgroups at full occupancy; the run reduction stays in registers
    "group_best": dict(names=("group_best_kernel",), exactly=1, equal={**CLEAN, LDS: 0}, at_most={"VGPRs": 64}),
    "group_split": dict(names=("group_split_kernel",), exactly=1, equal=CLEAN),
    "group_ids": dict(names=("group_ids_kernel",), exactly=1, equal=CLEAN),
    # 256-thread workgroups at full occupancy
    "after_cut": dict(names=("after_cut_kernel",), exactly=1, equal={**CLEAN, LDS: 0}, at_most={"VGPRs": 64}),
    "after_finish": dict(names=("after_finish_kernel",), exactly=1, equal=CLEAN),
    # 256-thread workgroups at full occupancy
    "boost_cut": dict(names=("boost_cut_kernel",), exactly=1, equal={**CLEAN, LDS: 0}, at_most={"VGPRs": 64}),
}

# The substrings the checks above and below pick their kernels by, in the order the families arrived: a kernel picked by one of them
# must match none of the earlier ones, or an older family's budget would silently apply to it (or its count be off).
FAMILY_SUBSTRINGS = ("stream_kernel", "batch_kernel", "multi_kernel", "stream_filter_kernel", "range_kernel", "row_vectors_kernel", "score_rows_kernel",
                     "group_best_kernel", "group_split_kernel", "group_ids_kernel", "after_cut_kernel", "after_finish_kernel", "facet_kernel",
                     "match_kernel", "boost_cut_kernel", "row_stats_kernel")


def _family(kernels, row):
    return {n: v for n, v in kernels.items() if any(s in n for s in row["names"]) and not any(s in n for s in row.get("unless", ()))}


@pytest.mark.parametrize("family", list(BUDGET))
def test_family_budget(family):
    row = BUDGET[family]
    mine = _family(resource_report(), row)
    if "exactly" in row:
        assert len(mine) == row["exactly"], sorted(mine)
    else:
        assert len(mine) >= row["at_least"], sorted(mine)
    for n, v in mine.items():
        for field, value in row.get("equal", {}).items():
            assert v[field] == value, (n, field, v)
        for field, limit in row.get("at_most", {}).items():
            assert v[field] <= limit, (n, field, v)


def test_later_kernels_match_no_earlier_family_substring():
    k = resource_report()
    for i, sub in enumerate(FAMILY_SUBSTRINGS):
        mine = [n for n in k if sub in n]
        assert mine, sub
        for n in mine:
            assert not any(s in n for s in FAMILY_SUBSTRINGS[:i]), (sub, n)


def test_facet_kernels_spill_no_sgprs():
    """No SGPR spill in any facet_kernel instantiation (the loop it shares with range_kernel fills the scalar register file: what the
    sink adds is read from the argument segment where it is used)."""
    k = resource_report()
    fac = {n: v for n, v in k.items() if "tkspmv12facet_kernel" in n}
    assert len(fac) >= 10, sorted(fac)
    for n, v in fac.items():
        assert v["SGPRs Spill"] == 0, (n, v["SGPRs Spill"])


def test_row_kernels_instantiations():
    """Which score_rows_kernel and row_stats_kernel instantiations exist: the 12-bit column layout, plain fp32 at 4 entries per lane
    (every column tier: no x in LDS), 8 entries per lane; row_stats_kernel in its four kinds each."""
    k = resource_report()
    sr, rs = [n for n in k if "score_rows_kernel" in n], [n for n in k if "row_stats_kernel" in n]
    layouts = [("4", "0"), ("4", "1"), ("8", "0")]
    assert sorted(re.search(r"score_rows_kernelILi(\d)ELb([01])E", n).groups() for n in sr) == layouts, sorted(sr)
    found = sorted(re.search(r"row_stats_kernelILi(\d)ELb([01])ELi(\d)E", n).groups() for n in rs)
    assert found == sorted((c, b, str(kind)) for c, b in layouts for kind in range(4)), sorted(rs)


def test_streaming_kernels_do_not_spill_and_fit_two_workgroups_per_cu():
    k = resource_report()
    stream = {n: v for n, v in k.items() if re.search(r"tkspmv1[23](stream|batch)_kernel", n)}
    multi = {n: v for n, v in k.items() if "tkspmv12multi_kernel" in n}
    assert len(stream) >= 30 and len(multi) == 12
    for n, v in {**stream, **multi}.items():
        tracing = re.search(r"stream_kernelILi4ELb0ELi1024ELi7ELi3ELb1E", n) or re.search(r"batch_kernelILi4ELi1024ELi[07]ELb1E", n)
        fused_tail = re.search(r"stream_kernelILi4ELb0ELi1024ELi[07]ELi3ELb[01]E", n)  # (a word of the selection tail; the loop is checked on the ISA below)
        if "kernelILi8E" not in n and not tracing and "batch_kernel" not in n and not fused_tail:  # (batch kernels: the ISA test below; the opt-in 8-entries-per-lane variants sit at the register limit; so do the tracing instantiations (TKSPMV_TRACE / TKSPMV_STATS runs only): the 12-bit layout's stream kernel, the batch kernels since round 3's checked thresholds)
            assert v["VGPRs Spill"] == 0, n
        assert v["AGPRs"] == 0, n
    for n, v in stream.items():
        dbg = bool(re.search(r"stream_kernelILi4ELb0ELi1024ELi0ELi3ELb1E", n))  # the tracing instantiation may keep a few stamps in scratch
        scores = "stream_kernelILi4ELb1E" in n or "stream_kernelILi8ELb1E" in n  # SpMV-only variants: one workgroup per CU is fine
        c8 = "kernelILi8E" in n
        dbg = dbg or bool(re.search(r"stream_kernelILi4ELb0ELi1024ELi7ELi3ELb1E", n)) or bool(re.search(r"batch_kernelILi4ELi1024ELi[07]ELb1E", n))
        # (the batch kernels call their selections and their repair phase as functions since round 4: the scratch size is those
        #  functions' stack; that the streaming loop itself touches no scratch is checked on the ISA below)
        if not dbg and not c8 and "batch_kernel" not in n:
            # (the single-query kernels keep a word or two of their selection tail in scratch; their loops are checked on the ISA too)
            assert v["ScratchSize [bytes/lane]"] <= (16 if "stream_kernelILi4ELb0ELi1024" in n else 0), (n, v)
        if not scores and not dbg:  # (the tracing instantiations of the single-query kernel may run one workgroup per CU)
            assert v["VGPRs"] <= 80, (n, v)
    # the headline kernels by name
    head = [n for n in stream if "12batch_kernelILi4ELi1024ELi7ELb0ELb0E" in n or "13stream_kernelILi4ELb0ELi1024ELi7ELi3ELb0E" in n
            or "12batch_kernelILi4ELi1024ELi7ELb0ELb1E" in n]
    assert len(head) == 3  # (the batch kernel of local thresholds, the exact one, the single-query stream kernel)
    for n, v in multi.items():
        q8 = "multi_kernelILi8E" in n
        assert v["VGPRs"] <= (128 if q8 else 80), (n, v)  # 8 queries per pass run 8-wave workgroups


def test_batch_kernels_stream_without_touching_scratch(tmp_path):
    """The batch kernel sits AT its register limit (80: two 576-thread workgroups per CU). Round 4 found out what one value too
    many costs: three reloads from scratch memory per packet and twice the time per query, with every functional test green.
    This compiles the instantiations on their own (seconds) and reads the ISA: no basic block that requests a packet
    (non-temporal load) or runs the fp32 segmented scan (v_add_f32_dpp) may contain a scratch instruction."""
    isa = compile_device_only(tmp_path, """#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels/common.hpp"
#include "kernels/select.hpp"
#include "kernels/packet_math.hpp"
#include "kernels/stream_kernel.hpp"
#include "kernels/local.hpp"
#include "kernels/batch_kernel.hpp"
namespace tkspmv {
#define INST(QM) template __global__ void batch_kernel<4, 1024, QM, false, false>(const BatchArgs); template __global__ void batch_kernel<4, 1024, QM, false, true>(const BatchArgs);
INST(0) INST(1) INST(2) INST(3) INST(4) INST(5) INST(6) INST(7) INST(8)
template __global__ void stream_kernel<4, false, 1024, 7, 3, false>(const StreamParams, const SelectParams);
template __global__ void stream_kernel<4, false, 1024, 0, 3, false>(const StreamParams, const SelectParams);
}
""")
    lines = isa.split("\n")
    starts = [i for i, ln in enumerate(lines) if (ln.startswith("_ZN6tkspmv12batch_kernel") or ln.startswith("_ZN6tkspmv13stream_kernel")) and "@" in ln]
    assert len(starts) == 20
    for start in starts:
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        blocks, cur = [], None
        for ln in lines[start:end]:
            if re.match(r"^\.LBB\d+_\d+:", ln):
                cur = {"name": ln.split(":")[0], "scratch": 0, "hot": False, "dpp": False, "max3": False}
                blocks.append(cur)
            elif cur is not None:
                if "scratch_" in ln:
                    cur["scratch"] += 1
                if ("global_load_dword" in ln or "buffer_load_dword" in ln) and " nt" in ln:  # (a packet request -- flat or, since round 5, buffer loads)
                    cur["hot"] = True
                # (the fp32 scan: DPP adds WITH the trigger's v_max3 behind them -- the server wave's sums of x use DPP adds too, round 5)
                cur["dpp"] = cur["dpp"] or "v_add_f32_dpp" in ln
                cur["max3"] = cur["max3"] or "v_max3_f32" in ln
        for b in blocks:
            b["hot"] = b["hot"] or (b["dpp"] and b["max3"])
        hot = [b for b in blocks if b["hot"]]
        assert len(hot) >= 3, "the streaming loop was not found in the ISA of " + lines[start].split(":")[0]
        assert all(b["scratch"] == 0 for b in hot), (lines[start].split(":")[0], [b for b in hot if b["scratch"]])


def test_no_chain_of_loads_waited_for_one_by_one(tmp_path):
    """Round 4 found the server wave staging x with sixteen loads each behind its own `s_waitcnt vmcnt(0)` -- sixteen trips through
    memory in a row, 6-16 us per query, invisible to every functional test (the compiler had put each 'in range ? load : 0' into a
    branch of its own). This compiles the headline kernels on their own and looks for runs of (wait for everything, ONE load) in
    the ISA: none of 6 or more may exist in the batch kernels (x staged with buffer loads since round 5: the resource's bounds check
    replaces clamped addresses, narrow x included), the single-query kernel and the multi-query kernels."""
    isa = compile_device_only(tmp_path, """#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels/common.hpp"
#include "kernels/select.hpp"
#include "kernels/packet_math.hpp"
#include "kernels/stream_kernel.hpp"
#include "kernels/local.hpp"
#include "kernels/batch_kernel.hpp"
#include "kernels/multi_kernel.hpp"
namespace tkspmv {
template __global__ void batch_kernel<4, 1024, 7, false, true>(const BatchArgs);
template __global__ void batch_kernel<4, 1024, 7, false, false>(const BatchArgs);
template __global__ void batch_kernel<4, 1024, 3, false, true>(const BatchArgs);
template __global__ void single_kernel<7>(const StreamParams, const SelectParams, const LocalParams);
template __global__ void multi_kernel<8, 0>(const StreamParams, const SelectParams, const MultiParams);
template __global__ void multi_kernel<4, 0>(const StreamParams, const SelectParams, const MultiParams);
}
""", (INCLUDE,))
    fn, seq, chains = None, [], {}

    def flush():
        if fn:
            chains[fn] = [len(m.group(0)) // 2 for m in re.finditer(r"(?:WL){6,}", "".join(seq))]

    for ln in isa.split("\n"):
        if re.match(r"^_ZN6tkspmv\w+:", ln):
            flush()
            fn, seq = ln.split(":")[0], []
        t = ln.strip().split(";")[0].strip()
        if not ln.startswith("\t") or not t:
            continue
        if t.startswith(("global_load", "buffer_load", "flat_load")):
            seq.append("L")
        elif t.startswith("s_waitcnt") and "vmcnt(0)" in t:
            seq.append("W")
        elif t.startswith(("global_store", "global_atomic", "s_sleep")):
            seq.append("x")
    flush()
    chains = {n: r for n, r in chains.items() if "select_kernel" not in n and "select_group_kernel" not in n}  # (non-template kernels of the headers)
    assert len(chains) == 6, sorted(chains)
    for name, runs in chains.items():  # (round 5: x is staged with buffer loads -- no clamped addresses --, the exact kernel has no such run either)
        assert len(runs) == 0, (name, runs)


def test_compact_batch_kernels_stream_without_touching_scratch(tmp_path):
    """The batch kernel's instantiations for the compact fp32 stream (QM_F32E5, csrc/wbscsr.hpp) sit at the register limit like the
    other batch kernels: their streaming loop touches no scratch memory either, read off the ISA of the two compiled on their own."""
    isa = compile_device_only(tmp_path, """#include <hip/hip_runtime.h>
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
""", (INCLUDE,))
    lines = isa.split("\n")
    starts = [i for i, ln in enumerate(lines) if ln.startswith(BUDGET["batch_f32e5"]["names"]) and "@" in ln]  # (the label line: "<name>:   ; @<name>")
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
