"""What a pass of column statistics costs, beside the load-only floor, the route through term predicates it replaces and a pass of
row statistics, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32; medians and spreads of --reps alternating measurements, bracketed by device events on a caller's
stream after warm-up (the method of row_stats_probe.py):
  col_nnz / col_max / col_min : one tkspmv_enqueue_col_stats pass of that kind over all rows (the memset of the output and, for MAX /
                                MIN, the closing launch included)
  col_nnz_mask50              : COL_NNZ among the rows of a 50 % allow-mask
  col_nnz_hot                 : COL_NNZ on a second matrix of the same shape in which column 0 is present in EVERY row: all 64 lanes of a
                                wave meet in one LDS word, the price of contention
  match_32                    : one tkspmv_enqueue_match call of 32 single-column predicates with their counts -- the route to 32
                                document frequencies before this kernel; a vocabulary of cols columns takes cols / 32 such calls
  match_half                  : one predicate whose clause half the rows satisfy (match_probe.py's leg), the upper end of the bracket an
                                unmasked COL_NNZ pass is expected in
  row_stats_l2sq              : one tkspmv_enqueue_row_stats pass, the yardstick that already exists
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix, in the same run. Recorded: us per leg, the column
plane's share of the floor, whether the bracket holds, and how many times one COL_NNZ call is faster than the cols / 32 match calls it
replaces. Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    L = mod._lib
    rows, cols, k = a.rows, 1024, 100
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    info = eng.info()
    # the same matrix with the first entry of every row moved to column 0
    hot_col = m.col.copy()
    hot_col[np.flatnonzero(np.concatenate(([True], m.row[1:] != m.row[:-1])))] = 0
    hot = mod.SpMV(m.row, hot_col, m.val, m.rows, m.cols, k=k, device=0)
    words = (rows + 31) // 32
    rng = np.random.default_rng(1)
    allow = rng.random(rows) < 0.5
    d_mask = torch.from_numpy(mod.row_mask(rows, allow).view(np.int32)).cuda()
    d_out = torch.zeros(cols, dtype=torch.int32, device="cuda")
    d_rows = torch.zeros(rows, dtype=torch.float32, device="cuda")
    # 32 single-column predicates over one table: clause bit b on column first32[b], query b asks for bit b
    first32 = np.arange(32) * (cols // 32)
    table = np.zeros(cols, dtype=np.uint32)
    table[first32] = np.uint32(1) << np.arange(32, dtype=np.uint32)
    preds = np.zeros((32, 4), dtype=np.uint32)
    preds[:, 0] = np.uint32(1) << np.arange(32, dtype=np.uint32)
    # ... and one clause that about half the rows satisfy (match_probe.py's recipe)
    p_col = np.bincount(m.col, minlength=cols) / max(1, rows)
    miss, chosen = 1.0, []
    for c in rng.permutation(cols):
        if miss <= 0.5:
            break
        chosen.append(c)
        miss *= 1.0 - min(0.99, p_col[c])
    half_t = np.zeros(cols, dtype=np.uint32)
    half_t[chosen] = 1
    d_table, d_half = torch.from_numpy(table.view(np.int32)).cuda(), torch.from_numpy(half_t.view(np.int32)).cuda()
    d_preds = torch.from_numpy(preds.view(np.int32)).cuda()
    d_masks = torch.zeros((32, words), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(32, dtype=torch.int32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    runs = {
        "col_nnz": lambda: eng.enqueue_col_stats(L.COL_NNZ, d_out.data_ptr(), stream=s),
        "col_max": lambda: eng.enqueue_col_stats(L.COL_MAX, d_out.data_ptr(), stream=s),
        "col_min": lambda: eng.enqueue_col_stats(L.COL_MIN, d_out.data_ptr(), stream=s),
        "col_nnz_mask50": lambda: eng.enqueue_col_stats(L.COL_NNZ, d_out.data_ptr(), masks=d_mask.data_ptr(), stream=s),
        "col_nnz_hot": lambda: hot.enqueue_col_stats(L.COL_NNZ, d_out.data_ptr(), stream=s),
        "match_32": lambda: eng.enqueue_match(d_table.data_ptr(), d_preds.data_ptr(), 32, d_masks.data_ptr(), out_stride=words, dev_counts=d_counts.data_ptr(),
                                              stream=s),
        "match_half": lambda: eng.enqueue_match(d_half.data_ptr(), d_preds.data_ptr(), 1, d_masks.data_ptr(), dev_counts=d_counts.data_ptr(), stream=s),
        "row_stats_l2sq": lambda: eng.enqueue_row_stats(L.ROW_L2SQ, d_rows.data_ptr(), stream=s),
    }
    # warm-up, and the legs are what the contract says
    checks = {"col_nnz": mod.col_stats(m, L.COL_NNZ), "col_max": mod.col_stats(m, L.COL_MAX).view(np.uint32), "col_min": mod.col_stats(m, L.COL_MIN).view(np.uint32),
              "col_nnz_mask50": mod.col_stats(m, L.COL_NNZ, allow), "col_nnz_hot": np.bincount(hot_col, minlength=cols).astype(np.uint32)}
    for name, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        if name in checks:
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), checks[name]), f"{name}: the device differs from host.col_stats"
        if name == "match_32":  # rows of the generator do not repeat these columns where the counts agree
            df32 = d_counts.cpu().numpy().view(np.uint32).copy()
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(timed(fn))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    # bytes of a packet and of its column plane: F32 at 8 entries per lane / F32C12 (at most 1024 columns) / F32
    packet_bytes, col_bytes = (3072.0, 1024.0) if info["packet_entries"] == 512 else ((1408.0, 384.0) if cols <= 1024 else (1536.0, 512.0))
    col_floor = floor * col_bytes / packet_bytes
    route = us["match_32"] * cols / 32.0  # the whole vocabulary through term predicates
    res = {"probe": "col_stats", "rows": rows, "cols": cols, "reps": a.reps,
           "us": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "stream_read_us": floor, "packet_bytes": packet_bytes, "column_plane_bytes": col_bytes, "column_plane_floor_us": col_floor,
           "col_nnz_inside_bracket": bool(col_floor <= us["col_nnz"] <= us["match_half"]),
           "match_route_us_for_all_columns": route,
           "match_route_over_col_nnz": route / us["col_nnz"],
           "hot_over_col_nnz": us["col_nnz_hot"] / us["col_nnz"],
           "mask50_over_col_nnz": us["col_nnz_mask50"] / us["col_nnz"],
           "col_nnz_over_row_stats_l2sq": us["col_nnz"] / us["row_stats_l2sq"],
           "nnz_minus_df_of_the_32_columns": [int(v) for v in (checks["col_nnz"][first32].astype(np.int64) - df32.astype(np.int64))],
           "packed_bytes": int(info["packed_bytes"])}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    hot.close()


if __name__ == "__main__":
    main()
