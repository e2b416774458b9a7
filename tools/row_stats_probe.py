"""What a pass of row statistics costs, beside the load-only floor and the way to the cosine weights without it, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32; medians and spreads of --reps alternating measurements. The device legs are bracketed by device
events on a caller's stream after warm-up (the method of score_rows_probe.py):
  row_stats_nnz / _l1 / _l2sq / _inv_l2 : one tkspmv_enqueue_row_stats pass of that kind (the memset of the output included)
  range_all_unpaced                     : one tkspmv_enqueue_range query whose threshold (-inf) every row with entries passes, all
                                          matches stored, on an engine created with RANGE_PERIOD=0 -- the upper end of the bracket
                                          the pass is expected in: it loads, multiplies, scans and stores 8 bytes per row, through
                                          the candidate lists
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix, in the same run. The host legs are wall-clock times:
  set_cosine_host_us     : SpMV.set_cosine() end to end (waits for the engine's stream, the pass, waits again)
  host_recipe_host_us    : host.cosine_weights(m) + SpMV.set_boost(weight=...), what answered the same question before: the COO in host
                           memory, float64 sums, an upload of rows floats
Recorded: us per pass, each pass as a fraction of the floor, the ratio of the two cosine installs. Prints one JSON line (and writes it
to --out when given)."""
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
    mod.set_option("RANGE_PERIOD", "0")
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    mod.set_option("RANGE_PERIOD", None)
    x = mod.create_sample_vector(cols, True, False, True, 100)
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros(rows, dtype=torch.float32, device="cuda")
    d_thr = torch.full((1,), float("-inf"), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_ri = torch.zeros(rows, dtype=torch.int32, device="cuda")
    d_rv = torch.zeros(rows, dtype=torch.float32, device="cuda")
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

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6  # us

    s = stream.cuda_stream
    kinds = {"nnz": L.ROW_NNZ, "l1": L.ROW_L1, "l2sq": L.ROW_L2SQ, "inv_l2": L.ROW_INV_L2}
    runs = {f"row_stats_{name}": (lambda kind=kind: timed(lambda: eng.enqueue_row_stats(kind, d_out.data_ptr(), stream=s))) for name, kind in kinds.items()}
    runs["range_all_unpaced"] = lambda: timed(lambda: eng.enqueue_range(d_x.data_ptr(), 1, d_thr.data_ptr(), d_cnt.data_ptr(), d_ri.data_ptr(), d_rv.data_ptr(),
                                                                       capacity=rows, stream=s))
    runs["set_cosine_host_us"] = lambda: wall(eng.set_cosine)
    runs["host_recipe_host_us"] = lambda: wall(lambda: eng.set_boost(weight=mod.cosine_weights(m)))
    for fn in runs.values():  # warm-up
        fn()
        torch.cuda.synchronize()
    stored = int(d_cnt.cpu().numpy()[0])
    # the two installs answer the same question: the weights agree within the float32 sums' error (test_row_stats_host.py has the bound)
    w_dev, w_host = eng.row_stats(L.ROW_INV_L2), mod.cosine_weights(m)
    rel = float(np.max(np.abs(w_dev.astype(np.float64) - w_host) / np.maximum(w_host, 1e-30)))
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(fn())
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "row_stats", "rows": rows, "cols": cols, "reps": a.reps,
           "us": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "stream_read_us": floor,
           "fraction_of_floor": {name: us[name] / floor for name in us if not name.endswith("_host_us")},
           "range_all_rows_stored": stored,
           "inside_bracket": {name: bool(floor <= us[name] <= us["range_all_unpaced"]) for name in us if name.startswith("row_stats_")},
           "host_recipe_over_set_cosine": us["host_recipe_host_us"] / us["set_cosine_host_us"],
           "max_rel_diff_device_vs_host_weights": rel,
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
