"""What the label sums -- the centroid update of k-means -- cost on the device, both sinks of the kernel side by side, beside the
load-only floor and the routes that existed before, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32; n_bins = 1, 8, 16, 64, 128 and 256 with labels from SpMV.assign against n_bins random vectors;
medians and spreads of --reps alternating measurements, every device leg bracketed by device events on a caller's stream after
warm-up (the method of assign_probe.py), the memset of the sums and the closing launch included:
  lds_<n>, direct_<n>  : one tkspmv_enqueue_label_sums call (RAW) with the LDS sink (ceil(n / 8) launches) / the direct sink forced
  float_<n>, unit_<n>  : the same with the sink the engine chooses and the FLOAT / UNIT closing launch
  index_add_<n>        : the device route of the parent commit -- torch.index_add_ over the COO keyed by labels[row] * cols + col
                         (the key's gather and arithmetic included): a float sum whose bits depend on the run
  host_<n>             : the recipe of INTEGRATION.md on the host's clock -- np.add.at in float64 over the COO --, --host-reps times
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix, in the same run. Recorded: us per call, each as a
multiple of the floor, the ratios between the routes, which sink is faster at every n_bins (what the engine's rule is set from), and
whether the routes agree: the two sinks' int64 sums as bits, both against Packed.label_sums for n_bins = 8 and 256, and the float
routes within fp32 summation error. Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = (1, 8, 16, 64, 128, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    L = mod._lib
    rows, cols = a.rows, 1024
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=100, device=0)
    e = eng.sums_exponent()
    xs = np.random.default_rng(5).standard_normal((max(BINS), cols)).astype(np.float32)
    labels = {n: eng.assign(xs[:n])[0] for n in BINS}
    d_lab = {n: torch.from_numpy(labels[n].view(np.int32)).cuda() for n in BINS}
    d_sums = torch.zeros(max(BINS) * cols, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(max(BINS) * cols, dtype=torch.float32, device="cuda")
    d_row = torch.from_numpy(m.row.astype(np.int64)).cuda()
    d_col = torch.from_numpy(m.col.astype(np.int64)).cuda()
    d_val = torch.from_numpy(m.val).cuda()
    d_acc = torch.zeros(max(BINS) * cols, dtype=torch.float32, device="cuda")
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

    def sums_call(n, mode, flags):
        eng.enqueue_label_sums(d_lab[n].data_ptr(), n, e, d_sums.data_ptr(), mode, d_out.data_ptr() if mode != L.SUMS_RAW else 0, flags, stream=s)

    def index_add(n):
        with torch.cuda.stream(stream):
            key = d_lab[n].to(torch.int64)[d_row] * cols + d_col
            d_acc[:n * cols].zero_()
            d_acc[:n * cols].index_add_(0, key, d_val)

    def host_route(n):
        t0 = time.perf_counter()
        acc = np.zeros(n * cols, dtype=np.float64)
        np.add.at(acc, labels[n].astype(np.int64)[m.row] * cols + m.col, m.val.astype(np.float64))
        return (time.perf_counter() - t0) * 1e6, acc

    runs = {}
    for n in BINS:
        runs[f"lds_{n}"] = lambda n=n: timed(lambda: sums_call(n, L.SUMS_RAW, L.SUMS_SINK_LDS))
        runs[f"direct_{n}"] = lambda n=n: timed(lambda: sums_call(n, L.SUMS_RAW, L.SUMS_SINK_DIRECT))
        runs[f"float_{n}"] = lambda n=n: timed(lambda: sums_call(n, L.SUMS_FLOAT, 0))
        runs[f"unit_{n}"] = lambda n=n: timed(lambda: sums_call(n, L.SUMS_UNIT, 0))
        runs[f"index_add_{n}"] = lambda n=n: timed(lambda: index_add(n))
    # warm-up, and the routes' answers side by side
    agree, host_us = {}, {}
    packed = mod.Packed(m, k=100, n_wave_partitions=eng.info()["n_wave_partitions"])
    for n in BINS:
        got = {}
        for sink in ("lds", "direct"):
            runs[f"{sink}_{n}"]()
            torch.cuda.synchronize()
            got[sink] = d_sums[:n * cols].cpu().numpy().copy()
        runs[f"float_{n}"]()
        torch.cuda.synchronize()
        f = d_out[:n * cols].cpu().numpy().astype(np.float64)
        runs[f"unit_{n}"]()
        runs[f"index_add_{n}"]()
        torch.cuda.synchronize()
        t = [host_route(n) for _ in range(a.host_reps)]
        host_us[str(n)] = float(np.median([x[0] for x in t]))
        ref = t[0][1]
        mag = np.zeros(n * cols)
        np.add.at(mag, labels[n].astype(np.int64)[m.row] * cols + m.col, np.abs(m.val).astype(np.float64))
        agree[str(n)] = {"sinks_equal_as_bits": bool(np.array_equal(got["lds"], got["direct"])),
                         "float_within_fp32_rounding_of_float64": bool(np.all(np.abs(f - ref) <= np.abs(ref) * 2.0 ** -23 + 1e-30)),
                         "index_add_max_error_over_fp32_bound": float(np.max(np.abs(d_acc[:n * cols].cpu().numpy() - ref) / (mag * 2.0 ** -24 * 20000 + 1e-30))),
                         "bins_used": int(np.unique(labels[n]).size)}
        if n in (8, 256):
            agree[str(n)]["sinks_equal_packed_twin"] = bool(np.array_equal(got["direct"], packed.label_sums(labels[n], n, e)[0].ravel()))
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(fn())
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "label_sums", "rows": rows, "cols": cols, "reps": a.reps, "host_reps": a.host_reps, "quantum_exp": e, "lds_bins_per_launch": 8,
           "us": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "host_us": host_us, "stream_read_us": floor,
           "over_floor": {name: us[name] / floor for name in us},
           "faster_sink": {str(n): "lds" if us[f"lds_{n}"] <= us[f"direct_{n}"] else "direct" for n in BINS},
           "direct_over_lds": {str(n): us[f"direct_{n}"] / us[f"lds_{n}"] for n in BINS},
           "index_add_over_unit": {str(n): us[f"index_add_{n}"] / us[f"unit_{n}"] for n in BINS},
           "host_over_unit": {str(n): host_us[str(n)] / us[f"unit_{n}"] for n in BINS},
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
