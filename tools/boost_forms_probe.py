"""Time per query of the boosted range, facet and grouped forms (tkspmv_enqueue_boosted_range / _facets / _grouped) beside the forms
they extend and beside a START page of boosted top-k, on the same engine, in ONE process. A probe, not a test; tools/boost_probe.py's
method.

1M x 1024, 20 nnz/row, gamma, fp32, k = 100, 4 stream copies, 200 back-to-back queries per leg (8 distinct vectors), each leg
bracketed by one pair of device events on a caller's stream after one warm-up call per leg; `rounds` rounds over all legs, the median
reported beside every round's figure (the spread). The boost is the cosine weights set_cosine() installs. Legs:
  range_100th / boosted_page          : the yardsticks -- enqueue_range at each vector's 100th best score, enqueue_boosted from the top
  boosted_range_100th / _median       : enqueue_boosted_range at each vector's 100th best and median cosine (capacity 4096 per query)
  facets_16 / boosted_facets_16       : enqueue_facets beside enqueue_boosted_facets at the median, 16 bins (the LDS regime)
  facets_8192 / boosted_facets_8192   : the same at 8192 bins (global atomics in the boosted form)
  grouped / boosted_grouped           : enqueue_grouped beside enqueue_boosted_grouped, 8192 groups
One relation follows from the code and is checked ("selective_range_below_boosted_page"): the selective boosted range query runs a
strict subset of the boosted page's launches -- scores and one array pass against scores, cut, five radix launches, select, finish.
Everything else is reported: the expected cost of a boosted form is a scores pass plus 12-16 MB of array traffic (4 bytes per row of
scores, weights and -- facets -- labels). One query of every leg is checked against the numpy restatement before anything is timed.
Prints one JSON line (and writes it to --out when given)."""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # (torch's HIP runtime initialises before the library's)
    torch.cuda.init()
    import _pkg
    mod = _pkg.load()
    rows, cols, k, n, distinct, cap = a.rows, 1024, 100, a.queries, 8, 4096
    m = mod.generate_matrix(rows, cols, 20, "gamma", 2)
    eng = mod.SpMV(m.row, m.col, m.val, m.rows, m.cols, k=k, device=0, stream_replicas=4)
    present = np.bincount(m.row, minlength=rows)[:rows] > 0
    rng = np.random.default_rng(3)
    labels = {16: rng.integers(0, 16, rows).astype(np.uint32), 8192: rng.integers(0, 8192, rows).astype(np.uint32)}
    eng.set_groups(labels[8192], 8192)
    eng.set_cosine()
    w = eng.row_stats(mod._lib.ROW_INV_L2)
    base = np.stack([mod.create_sample_vector(cols, True, False, True, 1000 + i) for i in range(distinct)]).astype(np.float32)
    ys, tau = [], {name: np.zeros(distinct, dtype=np.float32) for name in ("raw100", "rawmed", "cos100", "cosmed")}
    for i in range(distinct):  # each distinct vector's thresholds, from the engine's own scores
        eng.reset(base[i])
        ys.append(eng.scores().copy())
        raw = np.sort(ys[i][present])[::-1]
        cos = mod.boost_scores(ys[i], w)
        cos = np.sort(cos[present & (cos > -np.inf)])[::-1]
        tau["raw100"][i], tau["rawmed"][i], tau["cos100"][i], tau["cosmed"][i] = raw[99], raw[raw.size // 2], cos[99], cos[cos.size // 2]
    pick = np.arange(n) % distinct
    dxs = torch.from_numpy(base[pick]).cuda()
    dtau = {name: torch.from_numpy(t[pick]).cuda() for name, t in tau.items()}
    dlab = {nb: torch.from_numpy(lab.view(np.int32)).cuda() for nb, lab in labels.items()}
    out_i = torch.zeros((n, cap), dtype=torch.int32, device="cuda")
    out_v = torch.zeros((n, cap), dtype=torch.float32, device="cuda")
    out_g = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    out_n = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out_t = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out_c = torch.zeros((n, 8192), dtype=torch.int32, device="cuda")
    out_b = torch.zeros((n, 8192, 2), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()  # (the default stream's handle is 0, which the library reads as "the engine's stream")
    torch.cuda.synchronize()
    X, S = dxs.data_ptr(), stream.cuda_stream
    I, V, G, N, T, CN, BE = (t.data_ptr() for t in (out_i, out_v, out_g, out_n, out_t, out_c, out_b))

    def facets(nb, boosted):
        kw = dict(n_bins=nb, dev_labels=dlab[nb].data_ptr(), dev_best=BE, dev_totals=T, stream=S)
        if boosted:
            return lambda: eng.enqueue_boosted_facets(X, n, dtau["cosmed"].data_ptr(), CN, **kw)
        return lambda: eng.enqueue_facets(X, n, dtau["rawmed"].data_ptr(), CN, **kw)

    legs = [("range_100th", lambda: eng.enqueue_range(X, n, dtau["raw100"].data_ptr(), N, I, V, cap, stream=S)),
            ("boosted_page", lambda: eng.enqueue_boosted(X, n, dev_idx=I, dev_val=V, dev_n=N, dev_total=T, stream=S)),
            ("boosted_range_100th", lambda: eng.enqueue_boosted_range(X, n, dtau["cos100"].data_ptr(), N, dev_idx=I, dev_val=V, capacity=cap, stream=S)),
            ("boosted_range_median", lambda: eng.enqueue_boosted_range(X, n, dtau["cosmed"].data_ptr(), N, dev_idx=I, dev_val=V, capacity=cap, stream=S)),
            ("facets_16", facets(16, False)), ("boosted_facets_16", facets(16, True)),
            ("facets_8192", facets(8192, False)), ("boosted_facets_8192", facets(8192, True)),
            ("grouped", lambda: eng.enqueue_grouped(X, n, dev_idx=I, dev_val=V, dev_grp=G, dev_n=N, stream=S)),
            ("boosted_grouped", lambda: eng.enqueue_boosted_grouped(X, n, dev_idx=I, dev_val=V, dev_grp=G, dev_n=N, stream=S))]

    # warm-up (the first call allocates) and query 1 of every leg against the restatement
    y, q = ys[1], 1
    sb = mod.boost_scores(y, w)
    ok = present & (sb > -np.inf)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)

    def range_ok(want):
        cnt = int(u32(out_n)[q])
        kept = min(cnt, cap)
        got = set(zip(u32(out_i)[q, :kept].tolist(), u32(out_v)[q, :kept].tolist()))
        return cnt == want[2] and len(got) == kept and got <= set(zip(want[0].tolist(), want[1].view(np.uint32).tolist()))

    def facets_ok(nb, want):
        best = u32(out_b).reshape(-1, 2)[q * nb:(q + 1) * nb]  # (the call's own layout: [n][nb] records from the buffer's start)
        return bool(np.array_equal(u32(out_c).ravel()[q * nb:(q + 1) * nb], want[0]) and np.array_equal(best[:, 0], want[1]) and
                    np.array_equal(best[:, 1], want[2].view(np.uint32)) and int(u32(out_t)[q]) == want[3])

    def lists_ok(want):  # (the call's own layout: [n][k] entries from the buffers' start)
        return bool(np.array_equal(u32(out_i).ravel()[q * k:(q + 1) * k], want[0]) and np.array_equal(u32(out_v).ravel()[q * k:(q + 1) * k], want[1].view(np.uint32)))

    def grouped_ok(want):
        return lists_ok(want) and bool(np.array_equal(u32(out_g)[q], want[2]) and int(u32(out_n)[q]) == want[3])

    def page_ok(want):
        return lists_ok(want) and int(u32(out_n)[q]) == want[2]

    checks = {"range_100th": lambda: range_ok(mod.boosted_matches(y, present, tau["raw100"][q])),
              "boosted_page": lambda: page_ok(mod.page_after(sb, present, k)),
              "boosted_range_100th": lambda: range_ok(mod.boosted_matches(y, present, tau["cos100"][q], w)),
              "boosted_range_median": lambda: range_ok(mod.boosted_matches(y, present, tau["cosmed"][q], w)),
              "facets_16": lambda: facets_ok(16, mod.facet_counts(y, present, labels[16], 16, tau["rawmed"][q])),
              "boosted_facets_16": lambda: facets_ok(16, mod.facet_counts(sb, ok, labels[16], 16, tau["cosmed"][q])),
              "facets_8192": lambda: facets_ok(8192, mod.facet_counts(y, present, labels[8192], 8192, tau["rawmed"][q])),
              "boosted_facets_8192": lambda: facets_ok(8192, mod.facet_counts(sb, ok, labels[8192], 8192, tau["cosmed"][q])),
              "grouped": lambda: grouped_ok(mod.collapse_topk(y, present, labels[8192], k)),
              "boosted_grouped": lambda: grouped_ok(mod.collapse_topk(sb, ok, labels[8192], k))}
    checked = {}
    for name, fn in legs:
        fn()
        stream.synchronize()
        checked[name] = bool(checks[name]())
    us = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / n)  # us per query
    med = {name: float(np.median(v)) for name, v in us.items()}
    ratio = {"boosted_range_100th/range_100th": med["boosted_range_100th"] / med["range_100th"],
             "boosted_range_100th/boosted_page": med["boosted_range_100th"] / med["boosted_page"],
             "boosted_range_median/boosted_page": med["boosted_range_median"] / med["boosted_page"],
             "boosted_facets_16/facets_16": med["boosted_facets_16"] / med["facets_16"],
             "boosted_facets_8192/facets_8192": med["boosted_facets_8192"] / med["facets_8192"],
             "boosted_grouped/grouped": med["boosted_grouped"] / med["grouped"]}
    res = {"probe": "boost_forms", "device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "k": k, "queries": n, "rounds": a.rounds,
           "range_capacity": cap, "us_per_query_median": med, "us_per_query_rounds": us, "ratio": ratio,
           "selective_range_below_boosted_page": bool(all(r < p for r, p in zip(us["boosted_range_100th"], us["boosted_page"]))),
           "results_equal_restatement": checked}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
