"""What every row's n best vectors cost, beside the load-only floor, the single-best assignment and the route that existed before, in
ONE process.

1M x 1024, 20 nnz/row, gamma, fp32; count = 16, 64 and 256 random normal vectors; medians and spreads of --reps alternating
measurements, every leg bracketed by device events on a caller's stream after warm-up (the method of assign_probe.py):
  nearest_n<n>_<count>       : one tkspmv_enqueue_nearest call, n = 1, 2, 4 (the fill launch included): count / 16 passes over the matrix
  nearest_n1_masked_<count>  : the same with n = 1 under an allow-mask of half the rows
  assign_<count>             : one tkspmv_enqueue_assign call (its two memsets included), the yardstick for what the lists and the
                               merge cost
  score_rows_n<n>_<count>    : the route of the parent commit -- tkspmv_enqueue_score_rows over a list of ALL rows into a
                               [count][rows] device array, then torch.topk(n, dim=0) on the same stream
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix, in the same run. The two routes' answers are compared
first, and the probe fails unless they agree on every row: the scores as bits, the labels wherever no two of a row's scores are equal
(torch.topk promises no order among equals), and n = 1 unmasked equals enqueue_assign outright. Prints one JSON line (and writes it to
--out when given)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (16, 64, 256)
NS = (1, 2, 4)


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
    rows, cols = a.rows, 1024
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    xs = np.random.default_rng(5).standard_normal((max(COUNTS), cols)).astype(np.float32)
    allow = np.random.default_rng(6).random(rows) < 0.5
    d_xs = torch.from_numpy(xs).cuda()
    d_mask = torch.from_numpy(mod.row_mask(rows, allow).view(np.int32).copy()).cuda()
    d_lab = torch.zeros((rows, max(NS)), dtype=torch.int32, device="cuda")
    d_sc = torch.zeros((rows, max(NS)), dtype=torch.float32, device="cuda")
    d_alab = torch.zeros(rows, dtype=torch.int32, device="cuda")
    d_abest = torch.zeros(rows, dtype=torch.float32, device="cuda")
    d_rows = torch.arange(rows, dtype=torch.int32, device="cuda")
    d_scores = torch.zeros((max(COUNTS), rows), dtype=torch.float32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    old = {}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def new_route(count, n, masked=False):
        eng.enqueue_nearest(d_xs.data_ptr(), count, n, d_lab.data_ptr(), d_sc.data_ptr(), dev_mask=d_mask.data_ptr() if masked else 0, stream=s)

    def old_route(count, n):
        eng.enqueue_score_rows(d_xs.data_ptr(), count, d_rows.data_ptr(), rows, d_scores.data_ptr(), stream=s)
        with torch.cuda.stream(stream):
            old[count, n] = torch.topk(d_scores[:count], n, dim=0)

    runs = {}
    for count in COUNTS:
        for n in NS:
            runs[f"nearest_n{n}_{count}"] = lambda count=count, n=n: timed(lambda: new_route(count, n))
            runs[f"score_rows_n{n}_{count}"] = lambda count=count, n=n: timed(lambda: old_route(count, n))
        runs[f"nearest_n1_masked_{count}"] = lambda count=count: timed(lambda: new_route(count, 1, True))
        runs[f"assign_{count}"] = lambda count=count: timed(lambda: eng.enqueue_assign(d_xs.data_ptr(), count, d_alab.data_ptr(), d_abest.data_ptr(), stream=s))
    agree = {}
    for count in COUNTS:  # warm-up, and the routes' answers side by side
        runs[f"assign_{count}"]()
        torch.cuda.synchronize()
        a_lab, a_best = d_alab.cpu().numpy().view(np.uint32), d_abest.cpu().numpy()
        tied = None
        for n in NS:
            runs[f"nearest_n{n}_{count}"]()
            runs[f"score_rows_n{n}_{count}"]()
            torch.cuda.synchronize()
            lab, sc = d_lab.cpu().numpy().view(np.uint32).reshape(-1)[:rows * n].reshape(rows, n), d_sc.cpu().numpy().reshape(-1)[:rows * n].reshape(rows, n)
            o_sc, o_lab = old[count, n].values.cpu().numpy().T, old[count, n].indices.cpu().numpy().T.astype(np.uint32)
            if tied is None:  # (the [count][rows] scores are the same for every n)
                srt = np.sort(d_scores[:count].cpu().numpy(), axis=0)
                tied = np.any(srt[1:] == srt[:-1], axis=0)
                del srt
            rec = {"score_bits_equal": bool(np.array_equal(sc.view(np.uint32), np.ascontiguousarray(o_sc).view(np.uint32))),
                   "labels_equal_where_untied": bool(np.array_equal(lab[~tied], o_lab[~tied])), "tied_rows": int(np.count_nonzero(tied))}
            if n == 1:
                rec["equals_assign"] = bool(np.array_equal(lab[:, 0], a_lab) and np.array_equal(sc[:, 0].view(np.uint32), a_best.view(np.uint32)))
            agree[f"n{n}_{count}"] = rec
            assert rec["score_bits_equal"] and rec["labels_equal_where_untied"] and rec.get("equals_assign", True), (count, n, rec)
        runs[f"nearest_n1_masked_{count}"]()
        torch.cuda.synchronize()
        lab, sc = d_lab.cpu().numpy().view(np.uint32).reshape(-1)[:rows], d_sc.cpu().numpy().reshape(-1)[:rows]
        ok = bool(np.array_equal(lab, np.where(allow, a_lab, np.uint32(0xFFFFFFFF))) and np.array_equal(sc.view(np.uint32), np.where(allow, a_best, np.float32(-np.inf)).view(np.uint32)))
        agree[f"n1_masked_{count}"] = {"equals_assign_on_the_mask": ok}
        assert ok, (count, "masked")
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(fn())
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "nearest", "rows": rows, "cols": cols, "reps": a.reps, "vectors_per_pass": 16,
           "us": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "stream_read_us": floor,
           "nearest_pass_over_floor": {f"n{n}_{c}": us[f"nearest_n{n}_{c}"] / ((c + 15) // 16) / floor for c in COUNTS for n in NS},
           "nearest_over_assign": {f"n{n}_{c}": us[f"nearest_n{n}_{c}"] / us[f"assign_{c}"] for c in COUNTS for n in NS},
           "masked_over_unmasked": {str(c): us[f"nearest_n1_masked_{c}"] / us[f"nearest_n1_{c}"] for c in COUNTS},
           "score_rows_over_nearest": {f"n{n}_{c}": us[f"score_rows_n{n}_{c}"] / us[f"nearest_n{n}_{c}"] for c in COUNTS for n in NS},
           "routes_agree": agree,
           "packed_bytes": int(eng.info()["packed_bytes"])}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
