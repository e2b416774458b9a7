"""What a query by stored row costs beside the query itself, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, K = 100; 1024 random rows; medians and spreads of --reps alternating measurements, each
bracketed by device events on a caller's stream after warm-up. Three figures:
  row_vectors : tkspmv_enqueue_row_vectors of the 1024 rows (one launch of row_vectors_kernel), in us and us per row
  batch       : the tkspmv_enqueue_batch sequence over those same 1024 vectors on the same engine, in us and us per query
  similar     : tkspmv_run_similar of the 1024 rows on the host's clock (upload, row vectors, batch sequence, wait, copy out),
                per row, beside tkspmv_time_queries' time per query over the same vectors
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix. Extraction moves cols x 4 bytes per row and reads
one to a few packets, against a full pass over the matrix per query: "row_vectors_fraction_of_batch" records how small a part of
the sequence it is. Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    rows, cols, k, n = a.rows, 1024, 100, a.queries
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    ids = np.random.default_rng(3).integers(0, rows, n).astype(np.uint32)
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    d_xs = torch.zeros((n, cols), dtype=torch.float32, device="cuda")
    d_len = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def host_timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    runs = {
        "row_vectors": lambda: timed(lambda: eng.enqueue_row_vectors(d_ids.data_ptr(), n, d_xs.data_ptr(), d_len.data_ptr(), stream=stream.cuda_stream)),
        "batch": lambda: timed(lambda: eng.enqueue_batch(d_xs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr(), stream=stream.cuda_stream)),
        "similar": lambda: host_timed(lambda: eng.similar(ids)),
        "time_queries": lambda: eng.time_queries(d_xs.data_ptr(), n, n) * 1e-3 * n,
    }
    for fn in runs.values():  # warm-up (row_vectors first: the other legs read its output)
        fn()
        torch.cuda.synchronize()
    lens = d_len.cpu().numpy().view(np.uint32)
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(fn())
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "similar", "rows": rows, "cols": cols, "k": k, "queries": n, "reps": a.reps,
           "us_total": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "us_per_row": {name: us[name] / n for name in us},
           "row_vectors_fraction_of_batch": us["row_vectors"] / us["batch"],
           "similar_per_row_over_time_queries_per_query": us["similar"] / us["time_queries"],
           "stream_read_us": floor,
           "row_vectors_bytes_written": int(n) * cols * 4,
           "row_entries_min_median_max": [int(lens.min()), float(np.median(lens)), int(lens.max())]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
