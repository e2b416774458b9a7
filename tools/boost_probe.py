"""Time per START page of boosted top-k (tkspmv_enqueue_boosted) beside search-after paging (tkspmv_enqueue_after) on the same
engine, in ONE process. A probe, not a test.

1M x 1024, 20 nnz/row, gamma, fp32, k = 100, 200 back-to-back queries per leg (8 distinct vectors), each leg bracketed by one pair
of device events on a caller's stream after one warm-up call per leg. Legs, in this order:
  after_first      : tkspmv_enqueue_after from the top (the yardstick: a path the boost does not touch)
  boosted_shared   : weight and bias, boost_stride = 0 (one pair for every query)
  boosted_per_query: a per-query bias (boost_stride = rows, no weight): the hybrid-fusion form, 4 bytes per row and query more
  after_again      : the yardstick once more (what the box does between two runs of the same code)
"ratio" is each boosted leg over the mean of the two after legs; the fused kernel adds at most 12 bytes per row of traffic to a
query that moves about 130, so it should stay below 1.15. One query of each boosted leg is checked against the numpy restatement
(boost_scores + page_after over the engine's own score vector) before anything is timed. Prints one JSON line (and writes it to
--out when given)."""
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
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    rows, cols, k, n, distinct = a.rows, 1024, 100, a.queries, 8
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=4)
    base = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(distinct)]).astype(np.float32)
    dxs = torch.from_numpy(base[np.arange(n) % distinct]).cuda()
    out_i = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    out_n = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out_t = torch.zeros((n,), dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    dw = torch.rand((rows,), generator=gen, device="cuda", dtype=torch.float32) * 1.5 + 0.5      # [0.5, 2)
    db = torch.rand((n, rows), generator=gen, device="cuda", dtype=torch.float32) * 2.0 - 1.0    # [-1, 1), one row per query
    stream = torch.cuda.Stream()  # (the default stream's handle is 0, which the library reads as "the engine's stream")
    torch.cuda.synchronize()
    outs = (out_i.data_ptr(), out_v.data_ptr(), out_n.data_ptr(), out_t.data_ptr(), 0)

    def after():
        eng.enqueue_after(dxs.data_ptr(), n, 0, 0, 0, *outs, stream=stream.cuda_stream)

    def shared():
        eng.enqueue_boosted(dxs.data_ptr(), n, dw.data_ptr(), db.data_ptr(), 0, 0, 0, 0, *outs, stream=stream.cuda_stream)

    def per_query():
        eng.enqueue_boosted(dxs.data_ptr(), n, 0, db.data_ptr(), rows, 0, 0, 0, *outs, stream=stream.cuda_stream)

    legs = [("after_first", after), ("boosted_shared", shared), ("boosted_per_query", per_query), ("after_again", after)]
    # warm-up (the first call allocates) and one query of each boosted leg against the restatement
    present = np.bincount(m.row, minlength=rows)[:rows] > 0
    eng.reset(base[1])
    y = eng.scores().copy()
    w, b0, b1 = dw.cpu().numpy(), db[0].cpu().numpy(), db[1].cpu().numpy()
    checked = {}
    for name, fn in legs[:3]:
        fn()
        stream.synchronize()
        want = {"after_first": lambda: mod.page_after(y, present, k),
                "boosted_shared": lambda: mod.page_after(mod.boost_scores(y, w, b0), present, k),
                "boosted_per_query": lambda: mod.page_after(mod.boost_scores(y, None, b1), present, k)}[name]()
        gi, gv = out_i[1].cpu().numpy().view(np.uint32), out_v[1].cpu().numpy()
        checked[name] = bool(np.array_equal(gi, want[0]) and np.array_equal(gv.view(np.uint32), want[1].view(np.uint32)) and
                             int(out_n[1]) == want[2] and int(out_t.cpu().numpy().view(np.uint32)[1]) == want[3])
    us = {}
    for name, fn in legs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        us[name] = e0.elapsed_time(e1) * 1e3 / n  # us per query
    yard = 0.5 * (us["after_first"] + us["after_again"])
    res = {"probe": "boost", "device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "k": k, "queries": n, "us_per_query": us,
           "ratio": {name: us[name] / yard for name in ("boosted_shared", "boosted_per_query")},
           "ratio_to_after_first": {name: us[name] / us["after_first"] for name in ("boosted_shared", "boosted_per_query", "after_again")},
           "bound": 1.15, "pages_equal_restatement": checked}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
