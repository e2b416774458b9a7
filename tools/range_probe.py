"""Time per query of range queries (tkspmv_enqueue_range) beside the top-k paths of the same matrix, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, stream_replicas = 4, 256 back-to-back queries per sequence, bracketed by device events on a
caller's stream after warm-up; medians and spreads of --reps alternating measurements. Thresholds are taken per query from the
top-k results of the engines themselves (no oracle): the 100th best score, the 1000th best (a second engine with k = 1000), and
the median score of the first query's row scores (about half the rows pass). Legs:
  range_100 / range_1000 / range_half : range queries at those thresholds, default engine (RANGE_PERIOD unset)
  range_100_mask50                    : the selective threshold with a 50 % random allow-mask
  range_100_unpaced                   : an engine created with RANGE_PERIOD=0
  batch                               : tkspmv_enqueue_batch of the default engine (the headline path)
  batch0                              : tkspmv_enqueue_batch of an engine created with BATCH=0 (one exact launch per query)
  stream_read                         : tkspmv_time_stream_read (the load-only floor)
The one relation that follows from the code: range_100 does a strict subset of batch0's work per query in fewer launches, so its
median must not exceed batch0's (reported as "range_100_le_batch0"). Prints one JSON line (and writes it to --out when given)."""
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

    def engine(k_=k, **options):
        for name, v in options.items():
            mod.set_option(name, v)
        e = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k_, device=0, stream_replicas=4)
        for name in options:
            mod.set_option(name, None)
        return e

    eng = engine()
    eng_unpaced = engine(RANGE_PERIOD="0")
    eng_batch0 = engine(BATCH="0")
    xs = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(n)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros((n, 1000), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, 1000), dtype=torch.float32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    # thresholds from the engines' own top-k results
    eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    t100 = out_v.cpu().numpy().reshape(-1)[:n * k].reshape(n, k)[:, k - 1].copy()
    eng1000 = engine(1000)
    eng1000.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
    eng1000.synchronize()
    t1000 = out_v.cpu().numpy()[:, 999].copy()
    eng1000.close()
    eng.reset(xs[0])
    y = eng.scores()
    thalf = np.full(n, np.median(y[y > 0]), dtype=np.float32)
    thr = {"100": t100, "1000": t1000, "half": thalf}
    dthr = {name: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for name, v in thr.items()}
    cap = {"100": 1024, "1000": 4096, "half": rows}
    dcount = torch.zeros((n,), dtype=torch.int32, device="cuda")
    r_i = torch.zeros((n * 4096,), dtype=torch.int32, device="cuda")
    r_v = torch.zeros((n * 4096,), dtype=torch.float32, device="cuda")
    h_i = torch.zeros((n, rows), dtype=torch.int32, device="cuda")  # (every match of the half-the-rows leg is stored: 8 bytes per row)
    h_v = torch.zeros((n, rows), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(1)
    dmask = torch.from_numpy(mod.row_mask(rows, rng.random(rows) < 0.5).view(np.int32)).cuda()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per query

    def range_leg(e, name, mask=0):
        oi, ov = (h_i, h_v) if name == "half" else (r_i, r_v)
        return lambda: e.enqueue_range(dxs.data_ptr(), n, dthr[name].data_ptr(), dcount.data_ptr(), oi.data_ptr(), ov.data_ptr(), cap[name],
                                       mask, 0, stream=stream.cuda_stream)

    runs = {
        "batch": lambda: eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr(), stream=stream.cuda_stream),
        "batch0": lambda: eng_batch0.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr(), stream=stream.cuda_stream),
        "range_100": range_leg(eng, "100"),
        "range_100_unpaced": range_leg(eng_unpaced, "100"),
        "range_100_mask50": range_leg(eng, "100", dmask.data_ptr()),
        "range_1000": range_leg(eng, "1000"),
        "range_half": range_leg(eng, "half"),
    }
    matches = {}
    for name, fn in runs.items():  # warm-up, and what the range legs found
        fn()
        torch.cuda.synchronize()
        if name.startswith("range"):
            c = dcount.cpu().numpy().view(np.uint32)
            matches[name] = [int(c.min()), float(np.median(c)), int(c.max())]
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(timed(fn))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    period_ns = eng.debug_counters()["pace_period_ns"]
    res = {"probe": "range", "rows": rows, "cols": cols, "queries": n, "reps": a.reps, "us_per_query": us,
           "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "matches_min_median_max": matches, "stream_read_us": floor,
           "ratio_to_batch": {name: us[name] / us["batch"] for name in us if name.startswith("range")},
           "ratio_to_stream_read": {name: us[name] / floor for name in us},
           "range_100_le_batch0": bool(us["range_100"] <= us["batch0"]),
           "engine_pace_period_ns": int(period_ns)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for e in (eng, eng_unpaced, eng_batch0):
        e.close()


if __name__ == "__main__":
    main()
