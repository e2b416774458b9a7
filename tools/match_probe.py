"""Time per query of term predicates (tkspmv_enqueue_match) beside a selective range query of the same matrix, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, stream_replicas = 4, 256 back-to-back queries per sequence, bracketed by device events on a
caller's stream after warm-up; medians and spreads of --reps alternating measurements. Every query has a clause table of its own
(clause_stride = cols). Legs:
  range_100         : range queries at each query's 100th best score (taken from the engine's own top-k), the yardstick
  match_none        : one must clause that no column belongs to: no packet is expanded (the hot path alone)
  match_two         : two must clauses on two of the rarest columns (a few hundred matches: as selective as range_100)
  match_rare        : one must clause on a rare column (a different one per query; the generator's columns are nearly uniform, so
                      even the rarest occurs in almost 2 % of the rows -- matches_min_median_max says how many -- and, at a dozen rows
                      per packet, many packets hold a match)
  match_half        : one must clause on a set of columns that about half the rows touch
  match_not         : must_not alone on a rare column: every packet takes the full path and nearly every row matches
  match_rare_mask50 : match_rare with a 50 % random allow-mask
  stream_read       : tkspmv_time_stream_read (the load-only floor over whole packets)
The one relation that follows from the code: a selective match leg moves a strict subset of range_100's bytes and does less per
packet, so its median must come out below range_100's (reported as "match_rare_lt_range_100", and for the leg that is as selective
as range_100, "match_two_lt_range_100"). column_plane_floor_us is stream_read times the
share of a packet's bytes its column plane takes. Prints one JSON line (and writes it to --out when given)."""
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
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    rows, cols, k, n = a.rows, 1024, 100, a.queries
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=4)
    info = eng.info()
    words = (rows + 31) // 32
    xs = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(n)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    dthr = torch.from_numpy(np.ascontiguousarray(out_v.cpu().numpy()[:, k - 1], dtype=np.float32)).cuda()
    r_i = torch.zeros((n * 1024,), dtype=torch.int32, device="cuda")
    r_v = torch.zeros((n * 1024,), dtype=torch.float32, device="cuda")
    dcount = torch.zeros((n,), dtype=torch.int32, device="cuda")

    # per-query clause tables: clause bit 0 on a rare column / on a set of columns half the rows touch
    freq = np.bincount(m.col, minlength=cols)
    order = np.argsort(freq, kind="stable")
    order = order[freq[order] > 0]
    rng = np.random.default_rng(1)
    p_col = freq / max(1, rows)  # share of the rows a column occurs in (columns within a row are distinct or nearly so)
    rare_t = np.zeros((n, cols), dtype=np.uint32)
    half_t = np.zeros((n, cols), dtype=np.uint32)
    two_t = np.zeros((n, cols), dtype=np.uint32)
    for i in range(n):
        rare_t[i, order[i % 64]] = 1
        two_t[i, order[i % 64]] = 1
        two_t[i, order[(i + 7) % 64]] |= 2
        miss, chosen = 1.0, []
        for c in rng.permutation(cols):
            if miss <= 0.5:
                break
            chosen.append(c)
            miss *= 1.0 - min(0.99, p_col[c])
        half_t[i, chosen] = 1
    d_rare, d_half = torch.from_numpy(rare_t.view(np.int32)).cuda(), torch.from_numpy(half_t.view(np.int32)).cuda()
    d_two = torch.from_numpy(two_t.view(np.int32)).cuda()
    must_both = torch.from_numpy(np.tile(np.array([3, 0, 0, 0], dtype=np.uint32), (n, 1)).view(np.int32)).cuda()
    must_absent = torch.from_numpy(np.tile(np.array([4, 0, 0, 0], dtype=np.uint32), (n, 1)).view(np.int32)).cuda()  # (no column has clause bit 2)
    must = torch.from_numpy(np.tile(np.array([1, 0, 0, 0], dtype=np.uint32), (n, 1)).view(np.int32)).cuda()
    must_not = torch.from_numpy(np.tile(np.array([0, 1, 0, 0], dtype=np.uint32), (n, 1)).view(np.int32)).cuda()
    dout = torch.zeros((n, words), dtype=torch.int32, device="cuda")
    mcount = torch.zeros((n,), dtype=torch.int32, device="cuda")
    dmask = torch.from_numpy(mod.row_mask(rows, rng.random(rows) < 0.5).view(np.int32)).cuda()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per query

    def match_leg(tables, preds, mask=0):
        return lambda: eng.enqueue_match(tables.data_ptr(), preds.data_ptr(), n, dout.data_ptr(), out_stride=words, dev_counts=mcount.data_ptr(),
                                         clause_stride=cols, dev_mask=mask, stream=stream.cuda_stream)

    runs = {
        "range_100": lambda: eng.enqueue_range(dxs.data_ptr(), n, dthr.data_ptr(), dcount.data_ptr(), r_i.data_ptr(), r_v.data_ptr(), 1024, 0, 0,
                                               stream=stream.cuda_stream),
        "match_none": match_leg(d_rare, must_absent),
        "match_two": match_leg(d_two, must_both),
        "match_rare": match_leg(d_rare, must),
        "match_half": match_leg(d_half, must),
        "match_not": match_leg(d_rare, must_not),
        "match_rare_mask50": match_leg(d_rare, must, dmask.data_ptr()),
    }
    matches = {}
    for name, fn in runs.items():  # warm-up, and what the legs found
        fn()
        torch.cuda.synchronize()
        c = (dcount if name.startswith("range") else mcount).cpu().numpy().view(np.uint32)
        matches[name] = [int(c.min()), float(np.median(c)), int(c.max())]
    # the masks are what the contract says (first and last query of the rare leg, against the numpy restatement)
    runs["match_rare"]()
    torch.cuda.synchronize()
    got = dout.cpu().numpy().view(np.uint32)
    for i in (0, n - 1):
        exp = mod.row_mask(rows, mod.match_rows(m.row, m.col, rows, rare_t[i], (1, 0, 0, 0)))
        assert np.array_equal(got[i], exp), f"match_rare query {i}: the mask differs from match_rows"
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(timed(fn))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    # bytes of a packet and of its column plane: F32 at 8 entries per lane / F32C12 (at most 1024 columns) / F32
    packet_bytes, col_bytes = (3072.0, 1024.0) if info["packet_entries"] == 512 else ((1408.0, 384.0) if cols <= 1024 else (1536.0, 512.0))
    col_floor = floor * col_bytes / packet_bytes
    res = {"probe": "match", "rows": rows, "cols": cols, "queries": n, "reps": a.reps, "us_per_query": us,
           "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "matches_min_median_max": matches, "stream_read_us": floor, "packet_bytes": packet_bytes, "column_plane_bytes": col_bytes,
           "column_plane_floor_us": col_floor,
           "ratio_to_range_100": {name: us[name] / us["range_100"] for name in us},
           "ratio_to_stream_read": {name: us[name] / floor for name in us},
           "ratio_to_column_plane_floor": {name: us[name] / col_floor for name in us if name.startswith("match")},
           "match_rare_lt_range_100": bool(us["match_rare"] < us["range_100"]),
           "match_two_lt_range_100": bool(us["match_two"] < us["range_100"]),
           "library": os.path.basename(mod._lib.LIB_PATH)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
