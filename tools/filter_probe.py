"""Time per query of filtered top-k against the same engine's unfiltered exact sequence.

1M x 1024, 20 nnz/row, fp32, K = 100, stream_replicas = 4, 256 back-to-back queries. The engine is created with option BATCH=0,
so its unfiltered sequence (tkspmv_enqueue_batch) is one exact launch per query with deferred selection -- the launch scheme of
tkspmv_enqueue_filtered. Both sequences are bracketed by device events on the caller's stream after warm-up; the median of
--reps alternating measurements is reported. Prints one JSON line (and writes it to --out when given)."""
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
    mod.set_option("BATCH", "0")
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=4)
    mod.set_option("BATCH", None)
    xs = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(n)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(1)
    masks = {"all_ones": np.ones(rows, dtype=bool), "random_50": rng.random(rows) < 0.5, "random_0.1": rng.random(rows) < 0.001}
    dmask = {name: torch.from_numpy(mod.row_mask(rows, allow).view(np.int32)).cuda() for name, allow in masks.items()}
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream", unordered against
    #  events recorded on torch's side)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per query

    runs = {"unfiltered": lambda: eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr(), stream=stream.cuda_stream)}
    for name in masks:
        runs[name] = (lambda d: lambda: eng.enqueue_filtered(dxs.data_ptr(), n, d.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr(),
                                                             stream=stream.cuda_stream))(dmask[name])
    for fn in runs.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(timed(fn))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    res = {"probe": "filter", "rows": rows, "cols": cols, "k": k, "queries": n, "us_per_query": us,
           "ratio_to_unfiltered": {name: us[name] / us["unfiltered"] for name in masks},
           "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()}}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
