"""What assigning every row to its best-scoring vector costs, beside the load-only floor and the route that existed before, in ONE
process.

1M x 1024, 20 nnz/row, gamma, fp32; count = 16, 64 and 256 random normal vectors; medians and spreads of --reps alternating
measurements, every leg bracketed by device events on a caller's stream after warm-up (the method of row_stats_probe.py):
  assign_<count>     : one tkspmv_enqueue_assign call (the memsets of both outputs included): count / 16 passes over the matrix
  score_rows_<count> : the route of the parent commit -- tkspmv_enqueue_score_rows over a list of ALL rows into a [count][rows] device
                       array, then torch.max(dim=0) on the same stream for the scores and the labels
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix, in the same run. Recorded: us per call and per vector,
each call as a multiple of the floor per pass, the ratio of the two routes, and whether they agree (scores as bits; labels wherever
the best score is not tied). Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (16, 64, 256)


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
    d_xs = torch.from_numpy(xs).cuda()
    d_lab = torch.zeros(rows, dtype=torch.int32, device="cuda")
    d_best = torch.zeros(rows, dtype=torch.float32, device="cuda")
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

    def old_route(count):
        eng.enqueue_score_rows(d_xs.data_ptr(), count, d_rows.data_ptr(), rows, d_scores.data_ptr(), stream=s)
        with torch.cuda.stream(stream):
            old[count] = torch.max(d_scores[:count], dim=0)

    runs = {}
    for count in COUNTS:
        runs[f"assign_{count}"] = lambda count=count: timed(lambda: eng.enqueue_assign(d_xs.data_ptr(), count, d_lab.data_ptr(), d_best.data_ptr(), stream=s))
        runs[f"score_rows_{count}"] = lambda count=count: timed(lambda: old_route(count))
    agree = {}
    for count in COUNTS:  # warm-up, and the two routes' answers side by side
        runs[f"assign_{count}"]()
        runs[f"score_rows_{count}"]()
        torch.cuda.synchronize()
        lab, best = d_lab.cpu().numpy().view(np.uint32), d_best.cpu().numpy()
        o_best, o_lab = old[count].values.cpu().numpy(), old[count].indices.cpu().numpy()
        sc = d_scores[:count].cpu().numpy()
        tied = (sc == o_best[None, :]).sum(axis=0) > 1
        agree[str(count)] = {"best_bits_equal": bool(np.array_equal(best.view(np.uint32), o_best.view(np.uint32))),
                             "labels_equal_where_untied": bool(np.array_equal(lab[~tied], o_lab[~tied].astype(np.uint32))),
                             "tied_rows": int(np.count_nonzero(tied)), "labels_used": int(np.unique(lab).size)}
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(fn())
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "assign", "rows": rows, "cols": cols, "reps": a.reps, "vectors_per_pass": 16,
           "us": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "us_per_vector": {name: us[name] / int(name.rsplit("_", 1)[1]) for name in us},
           "stream_read_us": floor,
           "assign_pass_over_floor": {str(c): us[f"assign_{c}"] / ((c + 15) // 16) / floor for c in COUNTS},
           "score_rows_over_assign": {str(c): us[f"score_rows_{c}"] / us[f"assign_{c}"] for c in COUNTS},
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
