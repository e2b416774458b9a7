"""csrc/stream_format.hpp without a GPU: the one function that turns (descriptor precision, stream value type, packet entries,
columns) into the template arguments (C, XCOLS, QM) the engine's kernels are chosen by. A kernel of a larger x tier than the matrix
needs computes the same result, only slower, so no result check sees a wrong tier: this table does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approximate-spmv-topk_amd", "csrc")

COLS = [1, 1024, 1025, 4096, 4097, 16384]
TIERS = [1024, 1024, 4096, 4096, 16384, 16384]  # tier(cols) of COLS
FLAT = [1024] * 6

# (desc.precision, stream Precision, packet entries) -> C, XCOLS at each of COLS, QM
TABLE = [
    ("TKSPMV_F32", "F32C12", 256, 4, FLAT, 7),
    ("TKSPMV_F32", "F32", 512, 8, FLAT, 0),
    ("TKSPMV_F32", "F32", 256, 4, TIERS, 0),
    ("TKSPMV_Q1_7", "Q1_7", 256, 4, TIERS, 1),
    ("TKSPMV_Q1_7_WIDE", "Q1_7", 256, 4, TIERS, 2),
    ("TKSPMV_F16", "F16", 256, 4, TIERS, 3),
    ("TKSPMV_FIXED", "FIXED", 256, 4, TIERS, 4),
    ("TKSPMV_FIXED", "FIXED20", 256, 4, FLAT, 6),
    ("TKSPMV_FIXED", "FIXED26", 256, 4, FLAT, 8),
    ("TKSPMV_Q1_7_F32", "Q1_7_RND", 256, 4, TIERS, 5),
]
ILLEGAL = [
    ("TKSPMV_F16", "F32", 256),
    ("TKSPMV_F32", "F16", 256),
    ("TKSPMV_F32", "F32C12", 512),
    ("TKSPMV_Q1_7", "Q1_7", 512),
    ("TKSPMV_Q1_7_F32", "Q1_7", 256),
    ("TKSPMV_Q1_7_WIDE", "Q1_7_RND", 256),
    ("TKSPMV_FIXED", "F32", 256),
    ("TKSPMV_F32", "F32", 128),
]


def _run(tmp_path, cases):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    calls = "\n".join(f"    show(stream_format_of({api}, Precision::{stream}, {entries}u, {cols}u));" for api, stream, entries, cols in cases)
    src = tmp_path / "fmt.cpp"
    src.write_text('#include <cstdio>\n#include "stream_format.hpp"\nusing namespace tkspmv;\n'
                   'static void show(StreamFormat f) { if (f.c == 0) puts("no format"); else printf("%d %d %d\\n", f.c, f.xcols, f.qm); }\n'
                   "int main() {\n" + calls + "\n    return 0;\n}\n")
    exe = tmp_path / "fmt"
    subprocess.check_call([gxx, "-std=c++17", "-I" + CSRC, "-o", str(exe), str(src)])
    return subprocess.check_output([str(exe)]).decode().strip().split("\n")


def test_format_table(tmp_path):
    cases = [(api, stream, entries, cols) for api, stream, entries, _, _, _ in TABLE for cols in COLS]
    cases += [(api, stream, entries, cols) for api, stream, entries in ILLEGAL for cols in (1, 1024, 16384)]
    want = [f"{c} {xc} {qm}" for _, _, _, c, xcols, qm in TABLE for xc in xcols]
    want += ["no format"] * (3 * len(ILLEGAL))
    got = _run(tmp_path, cases)
    assert len(got) == len(cases)
    for case, g, w in zip(cases, got, want):
        assert g == w, (case, g, w)
    # the table holds the 22 formats the kernels are instantiated for, no more
    assert len({g for g in got if g != "no format"}) == 22


def test_format_list_and_predicates(tmp_path):
    """The X-macro list the dispatch is generated from names the same 22 formats, and the predicates select what each kernel family takes."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "list.cpp"
    src.write_text('#include <cstdio>\n#include "stream_format.hpp"\nusing namespace tkspmv;\nint main() {\n'
                   '#define X(C, XCOLS, QM) { constexpr StreamFormat f{C, XCOLS, QM}; printf("%d %d %d %d %d %d %d %d\\n", f.c, f.xcols, f.qm, '
                   "(int)is_fp32(f), (int)is_batchable(f), (int)has_tracing_twins(f), (int)has_single_kernel(f), value_type_of(f.qm)); }\n"
                   "    TKSPMV_STREAM_FORMATS(X)\n    return 0;\n}\n")
    exe = tmp_path / "list"
    subprocess.check_call([gxx, "-std=c++17", "-I" + CSRC, "-o", str(exe), str(src)])
    rows = [tuple(int(v) for v in ln.split()) for ln in subprocess.check_output([str(exe)]).decode().strip().split("\n")]
    fmts = [r[:3] for r in rows]
    want = {(c, xc, qm) for _, _, _, c, xcols, qm in TABLE for xc in xcols}
    assert len(fmts) == 22 and set(fmts) == want
    assert sorted(r[:3] for r in rows if r[3]) == [(4, 1024, 0), (4, 1024, 7), (4, 4096, 0), (4, 16384, 0), (8, 1024, 0)]  # filter, range, row vectors
    assert sum(r[4] for r in rows) == 10 and all(r[1] == 1024 for r in rows if r[4])  # batch_kernel
    assert sorted(r[:3] for r in rows if r[5]) == [(4, 1024, 0), (4, 1024, 7)]  # tracing twins
    assert sorted(r[:3] for r in rows if r[6]) == [(4, 1024, 0), (4, 1024, 7)]  # single_kernel
    assert {r[2]: r[7] for r in rows} == {0: 0, 1: 1, 2: 1, 3: 2, 4: 0, 5: 1, 6: 3, 7: 4, 8: 6}  # value type of each mode
