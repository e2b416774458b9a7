"""Time per query of grouped top-k (tkspmv_enqueue_grouped) beside the exact top-k sequence of the same matrix, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, k = 100, stream_replicas = 4, 256 back-to-back queries per sequence, bracketed by device events
on a caller's stream after warm-up; medians and spreads of --reps alternating measurements. Legs:
  batch0            : tkspmv_enqueue_batch of an engine created with BATCH=0 (one exact launch per query)
  scores_only       : the SpMV-only kernel alone (tkspmv_profile's scores_kernel_ns; the engine's own stream)
  grouped_runs8     : grouped, contiguous groups of 8 rows (the common case: a document's passages are stored together)
  grouped_identity  : grouped, group = row (every lane a run of its own, as many groups as rows)
  grouped_scattered : grouped, label = row % 125000 (one atomic per eligible row, 8 rows per group far apart)
  grouped_one       : grouped, one group (every wave's maximum meets in one word)
  stream_read       : tkspmv_time_stream_read (the load-only floor)
"reduction_us" is grouped - scores_only: what the reduction to groups and the selection over them cost. The one relation that
follows from the code: a grouped query runs the scores kernel and more, so it cannot cost less than scores_only
("grouped_ge_scores_only"; if it is false, the probe is wrong). Prints one JSON line (and writes it to --out when given)."""
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
    eng_batch0 = engine(BATCH="0")
    xs = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(n)]).astype(np.float32)
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    out_g = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_n = torch.zeros((n,), dtype=torch.int32, device="cuda")
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    r = np.arange(rows)
    labelings = {"runs8": r // 8, "identity": r, "scattered": r % max(1, rows // 8), "one": np.zeros(rows, dtype=np.int64)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per query

    def grouped():
        eng.enqueue_grouped(dxs.data_ptr(), n, 0, 0, out_i.data_ptr(), out_v.data_ptr(), out_g.data_ptr(), out_n.data_ptr(), stream=stream.cuda_stream)

    def batch0():
        eng_batch0.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr(), stream=stream.cuda_stream)

    def scores_only():
        return eng.profile(dxs.data_ptr(), n, n)["scores_kernel_ns"] * 1e-3

    legs = ["batch0", "scores_only"] + ["grouped_" + name for name in labelings]
    found = {}
    for name, labels in labelings.items():  # warm-up, and how many groups each labeling's queries found
        eng.set_groups(labels)
        grouped()
        torch.cuda.synchronize()
        c = out_n.cpu().numpy()
        found["grouped_" + name] = [int(c.min()), int(c.max())]
    batch0()
    scores_only()
    torch.cuda.synchronize()
    samples = {name: [] for name in legs}
    for _ in range(a.reps):
        samples["batch0"].append(timed(batch0))
        samples["scores_only"].append(scores_only())
        for name, labels in labelings.items():
            eng.set_groups(labels)  # (waits for the engine's stream; the caller's stream was waited for by timed())
            samples["grouped_" + name].append(timed(grouped))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "grouped", "rows": rows, "cols": cols, "k": k, "queries": n, "reps": a.reps, "us_per_query": us,
           "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "entries_min_max": found, "stream_read_us": floor,
           "reduction_us": {name: us[name] - us["scores_only"] for name in us if name.startswith("grouped")},
           "ratio_to_batch0": {name: us[name] / us["batch0"] for name in us if name.startswith("grouped")},
           "grouped_ge_scores_only": bool(all(us[name] >= us["scores_only"] for name in us if name.startswith("grouped")))}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for e in (eng, eng_batch0):
        e.close()


if __name__ == "__main__":
    main()
