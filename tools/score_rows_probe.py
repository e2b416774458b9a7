"""What the scores of GIVEN rows cost, beside the way to get them without tkspmv_enqueue_score_rows, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, K = 100; 32 queries; medians and spreads of --reps alternating measurements, each bracketed by
device events on a caller's stream after warm-up. Legs:
  filtered_R      : tkspmv_enqueue_filtered of the 32 queries with the allow-mask of R random rows (R = 1024): a full pass over the
                    matrix per query -- what answers "what do these rows score?" without score_rows (for K of them at a time)
  score_rows_R    : tkspmv_enqueue_score_rows of the 32 queries over ONE list of R random rows, R = 128, 1024, 16384
  score_rows_per_query_1024 : the same with a list of 1024 rows per query
and tkspmv_time_stream_read, the load-only floor of one pass over the matrix. Recorded: us per call, us per (row, query), and
"score_rows_fraction_of_filtered" (both at R = 1024). Prints one JSON line (and writes it to --out when given)."""
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
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    rows, cols, k, nq = a.rows, 1024, 100, a.queries
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0)
    rng = np.random.default_rng(3)
    xs = np.stack([mod.create_sample_vector(cols, True, False, True, 100 + i) for i in range(nq)])
    d_xs = torch.from_numpy(xs).cuda()
    sizes = (128, 1024, 16384)
    lists = {R: rng.choice(rows, R, replace=False).astype(np.uint32) for R in sizes}
    d_lists = {R: torch.from_numpy(v.view(np.int32)).cuda() for R, v in lists.items()}
    per_query = np.stack([rng.choice(rows, 1024, replace=False).astype(np.uint32) for _ in range(nq)])
    d_per_query = torch.from_numpy(per_query.view(np.int32)).cuda()
    allow = np.zeros(rows, dtype=bool)
    allow[lists[1024]] = True
    d_mask = torch.from_numpy(mod.row_mask(rows, allow).view(np.int32)).cuda()
    d_scores = torch.zeros((nq, max(sizes)), dtype=torch.float32, device="cuda")
    out_i = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
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

    s = stream.cuda_stream
    runs = {"filtered_1024": lambda: timed(lambda: eng.enqueue_filtered(d_xs.data_ptr(), nq, d_mask.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr(), stream=s))}
    pairs = {"filtered_1024": 1024 * nq}
    for R in sizes:
        runs[f"score_rows_{R}"] = (lambda R=R: timed(lambda: eng.enqueue_score_rows(d_xs.data_ptr(), nq, d_lists[R].data_ptr(), R, d_scores.data_ptr(), stream=s)))
        pairs[f"score_rows_{R}"] = R * nq
    runs["score_rows_per_query_1024"] = lambda: timed(lambda: eng.enqueue_score_rows(d_xs.data_ptr(), nq, d_per_query.data_ptr(), 1024, d_scores.data_ptr(),
                                                                                   rows_stride=1024, stream=s))
    pairs["score_rows_per_query_1024"] = 1024 * nq
    for fn in runs.values():  # warm-up
        fn()
        torch.cuda.synchronize()
    # the two R = 1024 legs answer the same question: the filtered lists' scores are among score_rows' (same bits)
    eng.enqueue_score_rows(d_xs.data_ptr(), nq, d_lists[1024].data_ptr(), 1024, d_scores.data_ptr(), stream=s)
    eng.enqueue_filtered(d_xs.data_ptr(), nq, d_mask.data_ptr(), 0, out_i.data_ptr(), out_v.data_ptr(), stream=s)
    stream.synchronize()
    sc, fi, fv = d_scores.cpu().numpy()[:, :1024], out_i.cpu().numpy().view(np.uint32), out_v.cpu().numpy()
    pos = {int(r): j for j, r in enumerate(lists[1024])}
    agree = all(fv[q, j] == 0.0 or sc[q, pos[int(fi[q, j])]].view(np.uint32) == fv[q, j].view(np.uint32) for q in range(nq) for j in range(k))
    samples = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            samples[name].append(fn())
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "score_rows", "rows": rows, "cols": cols, "k": k, "queries": nq, "reps": a.reps,
           "us_per_call": us, "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "us_per_row_and_query": {name: us[name] / pairs[name] for name in us},
           "score_rows_fraction_of_filtered": us["score_rows_1024"] / us["filtered_1024"],
           "filtered_scores_equal_score_rows_bits": bool(agree),
           "stream_read_us": floor, "packed_bytes": int(eng.info()["packed_bytes"])}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
