"""Time per query of search-after paging (tkspmv_enqueue_after) beside the exact top-k sequence of the same matrix, in ONE process.

1M x 1024, 20 nnz/row, gamma, fp32, k = 100, stream_replicas = 4, 256 back-to-back queries per sequence (8 distinct vectors, each
with its own cursors), bracketed by device events on a caller's stream after warm-up; medians and spreads of --reps alternating
measurements. Legs:
  batch0           : tkspmv_enqueue_batch of an engine created with BATCH=0 (one exact launch per query)
  scores_only      : the SpMV-only kernel alone (tkspmv_profile's scores_kernel_ns; the engine's own stream)
  after_start      : a page from the top (dev_cursors = NULL)
  after_rank1000   : the page behind the query's 1000th row
  after_rank100000 : the page behind the query's 100 000th row (a tenth of the matrix is cut: that many predicated stores)
  after_mask50     : a page from the top under an allow-mask of half the rows
  stream_read      : tkspmv_time_stream_read (the load-only floor)
"paging_us" is after - scores_only: what the cut, the radix select over all rows, the selection and the bookkeeping cost. The one
relation that follows from the code: an after query runs the scores kernel and more, so it cannot cost less than scores_only
("after_ge_scores_only"; if it is false, the probe is wrong). Prints one JSON line (and writes it to --out when given)."""
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
    rows, cols, k, n, distinct = a.rows, 1024, 100, a.queries, 8
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
    base = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(distinct)]).astype(np.float32)
    xs = base[np.arange(n) % distinct]
    dxs = torch.from_numpy(xs).cuda()
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    out_n = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out_t = torch.zeros((n,), dtype=torch.int32, device="cuda")
    # the cursors behind rank R of every distinct vector, from the engine's own full score vector
    present = np.bincount(m.row, minlength=rows)[:rows] > 0
    ranks = [r for r in (1000, 100_000) if r < rows]
    cursors = {r: np.zeros((n, 4), dtype=np.uint32) for r in ranks}
    for i in range(distinct):
        eng.reset(base[i])
        y = eng.scores().copy()
        for r in ranks:
            cursors[r][i::distinct, :3] = mod.page_after(y, present, r)[4]
    dcur = {r: torch.from_numpy(c.view(np.int32)).cuda() for r, c in cursors.items()}
    dmask = torch.from_numpy(mod.row_mask(rows, np.random.default_rng(1).random(rows) < 0.5).view(np.int32)).cuda()
    # (a stream of its own: the default stream's handle is 0, which the library reads as "the engine's stream")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per query

    def after(dev_cursors=0, dev_mask=0):
        return lambda: eng.enqueue_after(dxs.data_ptr(), n, dev_cursors, dev_mask, 0, out_i.data_ptr(), out_v.data_ptr(), out_n.data_ptr(),
                                         out_t.data_ptr(), 0, stream=stream.cuda_stream)

    def batch0():
        eng_batch0.enqueue_batch(dxs.data_ptr(), n, out_i.data_ptr(), out_v.data_ptr(), stream=stream.cuda_stream)

    def scores_only():
        return eng.profile(dxs.data_ptr(), n, n)["scores_kernel_ns"] * 1e-3

    after_legs = {"after_start": after()}
    for r in ranks:
        after_legs[f"after_rank{r}"] = after(dcur[r].data_ptr())
    after_legs["after_mask50"] = after(0, dmask.data_ptr())
    left = {}
    for name, fn in after_legs.items():  # warm-up (the first call allocates), and the hits left behind each leg's cursors
        fn()
        torch.cuda.synchronize()
        t = out_t.cpu().numpy().view(np.uint32)
        left[name] = [int(t.min()), int(t.max())]
    batch0()
    scores_only()
    torch.cuda.synchronize()
    samples = {name: [] for name in ["batch0", "scores_only"] + list(after_legs)}
    for _ in range(a.reps):
        samples["batch0"].append(timed(batch0))
        samples["scores_only"].append(scores_only())
        for name, fn in after_legs.items():
            samples[name].append(timed(fn))
    us = {name: float(np.median(v)) for name, v in samples.items()}
    floor = eng.time_stream_read(64) * 1e-3
    res = {"probe": "after", "rows": rows, "cols": cols, "k": k, "queries": n, "reps": a.reps, "us_per_query": us,
           "spread_us": {name: [float(min(v)), float(max(v))] for name, v in samples.items()},
           "total_min_max": left, "stream_read_us": floor,
           "paging_us": {name: us[name] - us["scores_only"] for name in after_legs},
           "ratio_to_batch0": {name: us[name] / us["batch0"] for name in after_legs},
           "after_ge_scores_only": bool(all(us[name] >= us["scores_only"] for name in after_legs))}
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
