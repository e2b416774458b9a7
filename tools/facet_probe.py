"""Time per query of facet counts (tkspmv_enqueue_facets) beside the range queries of the same matrix, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, stream_replicas = 4, 256 back-to-back queries per sequence, bracketed by device events on a
caller's stream after warm-up; medians and spreads of --reps alternating measurements. Thresholds, per query where they depend on
it: the 100th best score (from the engine's own top-k results), the median score of the first query's row scores (about half the
rows pass) and -inf (every row with entries). Legs:
  range_count_<t>             : enqueue_range with capacity = 0 (count only: the yardstick) at t = 100 / half / minf
  range_full_half             : enqueue_range storing every match at the median score (what callers did for facets so far)
  facets_<t>_<bins>[_best]    : enqueue_facets with 16, 1024 and 1M bins (labels r % bins), without and with dev_best
  facets_<t>_16[_best]_global : the 16-bin legs on an engine created with FACET_LDS_BINS=0 (global atomics instead of the LDS histogram)
Two relations follow from the code and are reported as booleans: at half and minf with 16 bins the LDS regime is not slower than the
global one on the same input ("lds_not_slower"), and at half the 16-bin facets are faster than range_full_half, because nothing is
written per match ("facets16_faster_than_range_full"). Prints one JSON line (and writes it to --out when given)."""
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

    def engine(**options):
        for name, v in options.items():
            mod.set_option(name, v)
        e = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=4)
        for name in options:
            mod.set_option(name, None)
        return e

    eng = engine()
    eng_global = engine(FACET_LDS_BINS="0")
    xs = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(n)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr())
    eng.synchronize()
    t100 = out_v.cpu().numpy()[:, k - 1].copy()
    eng.reset(xs[0])
    y = eng.scores()
    thr = {"100": t100, "half": np.full(n, np.median(y[y > 0]), dtype=np.float32), "minf": np.full(n, -np.inf, dtype=np.float32)}
    dthr = {name: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for name, v in thr.items()}
    bins = {"16": 16, "1024": 1024, "1M": 1_000_000}
    dlab = {name: torch.from_numpy((np.arange(rows, dtype=np.int64) % b).astype(np.uint32).view(np.int32)).cuda() for name, b in bins.items()}
    dcount = torch.zeros((n,), dtype=torch.int32, device="cuda")
    h_i = torch.zeros((n, rows), dtype=torch.int32, device="cuda")  # (every match of range_full_half is stored: 8 bytes per row)
    h_v = torch.zeros((n, rows), dtype=torch.float32, device="cuda")
    f_counts = torch.zeros((n * max(bins.values()),), dtype=torch.int32, device="cuda")
    f_best = torch.zeros((n * max(bins.values()),), dtype=torch.int64, device="cuda")
    f_totals = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per query

    def facet_leg(e, t, b, best):
        return lambda: e.enqueue_facets(dxs.data_ptr(), n, dthr[t].data_ptr(), f_counts.data_ptr(), bins[b], dlab[b].data_ptr(),
                                        f_best.data_ptr() if best else 0, f_totals.data_ptr(), stream=stream.cuda_stream)

    runs = {}
    for t in thr:
        runs[f"range_count_{t}"] = (lambda t=t: eng.enqueue_range(dxs.data_ptr(), n, dthr[t].data_ptr(), dcount.data_ptr(), stream=stream.cuda_stream))
    runs["range_full_half"] = lambda: eng.enqueue_range(dxs.data_ptr(), n, dthr["half"].data_ptr(), dcount.data_ptr(), h_i.data_ptr(), h_v.data_ptr(), rows,
                                                        stream=stream.cuda_stream)
    for t in thr:
        for b in bins:
            for best in (False, True):
                runs[f"facets_{t}_{b}" + ("_best" if best else "")] = facet_leg(eng, t, b, best)
        for best in (False, True):
            runs[f"facets_{t}_16" + ("_best" if best else "") + "_global"] = facet_leg(eng_global, t, "16", best)
    matches = {}
    for name, fn in runs.items():  # warm-up, and what the legs found
        fn()
        torch.cuda.synchronize()
        c = (dcount if name.startswith("range") else f_totals).cpu().numpy().view(np.uint32)
        matches[name] = [int(c.min()), float(np.median(c)), int(c.max())]
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(timed(fn))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    lds_not_slower = {f"{t}{s}": bool(us[f"facets_{t}_16{s}"] <= us[f"facets_{t}_16{s}_global"]) for t in ("half", "minf") for s in ("", "_best")}
    res = {"probe": "facets", "rows": rows, "cols": cols, "queries": n, "reps": a.reps, "us_per_query": us,
           "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "matches_min_median_max": matches,
           "lds_not_slower": lds_not_slower,
           "facets16_faster_than_range_full": {s or "counts": bool(us[f"facets_half_16{s}"] < us["range_full_half"]) for s in ("", "_best")},
           "engine_pace_period_ns": int(eng.debug_counters()["pace_period_ns"])}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    eng_global.close()


if __name__ == "__main__":
    main()
