"""Worker of tests/test_gpu_dist_batch.py::test_two_ranks_on_one_gpu_through_the_pipelined_step: rank RANK of WORLD_SIZE, all on
cuda:0, process group over gloo; the native pipelined step with the all-gather staged through the host.
A second argument "short-shards" selects the worker of test_two_ranks_on_short_signed_shards_through_the_pipelined_step."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pkg  # noqa: E402
import oracle_lib as O  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    mod = _pkg.load()
    from importlib import import_module
    dmod = import_module("approximate_spmv_topk_amd.distributed")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    k, rows, n_x, n_queries = 100, 300000, 40, 75
    shard, (r0, r1), total_nnz = dmod.generate_shard(rows, 1024, 20, "gamma", 2, rank, world)
    xs = np.stack([mod.create_sample_vector(1024, True, False, True, 9000 + i) for i in range(n_x)])
    dxs = torch.from_numpy(xs).to(dev)
    eng = mod.SpMV(shard.row, shard.col, shard.val, shard.rows, shard.cols, k=k, device=0, first_row=r0)
    step = dmod.NativeShardedSpMV(eng, dev, host_exchange=True)
    assert step.world == world
    whole = mod.generate_matrix(rows, 1024, 20, "gamma", 2)
    assert whole.nnz == total_nnz

    def check(q_index, idx, val):
        x = xs[q_index % n_x]
        gi, gv = O.gold_topk(whole.row, whole.col, whole.val, x, k)
        assert set(idx.tolist()) == set(gi.tolist()), f"query {q_index}: index set differs from the gold over the whole matrix"
        assert np.allclose(np.sort(val)[::-1], np.sort(gv)[::-1], rtol=1e-4, atol=0)

    # 75 queries = two full exchange batches + a partial one of 11 (buffer sets 0, 1, 0)
    step.run_many(dxs.data_ptr(), n_x, 64)
    vb, ib = step.read_batch()  # the second batch: queries 32..63
    assert vb.shape[0] == 32
    for j in (0, 13, 31):
        check(32 + j, ib[j], vb[j])
    for i in range(64, n_queries):
        step.enqueue(dxs[i % n_x].data_ptr())
    vb, ib = step.read_batch()  # flushes the open batch of 11
    assert vb.shape[0] == n_queries - 64
    for j in range(vb.shape[0]):
        check(64 + j, ib[j], vb[j])
    v, i = step.read()
    assert np.array_equal(i, ib[-1]) and np.array_equal(v, vb[-1])
    # exchange batches of 1 (every query on its own) and of 5
    for batch, n in ((1, 3), (5, 12)):
        step.set_batch(batch)
        step.run_many(dxs.data_ptr(), n_x, n)
        vb, ib = step.read_batch()
        last_n = n % batch or batch
        assert vb.shape[0] == last_n
        for j in range(last_n):
            check(n - last_n + j, ib[j], vb[j])
    step.close()
    eng.close()
    dist.barrier()
    dist.destroy_process_group()
    print("REHEARSAL_OK", rank)


def main_short_shards():
    """Rank 0 on rows [0, 37) and rank 1 on rows [37, 3000) of the signed matrix, k = 100, min_score = -1e30: rank 0's lists end in
    63 fillers, which must stay behind rank 1's negative scores. 11 queries in exchange batches of 4; every list of the last batch
    equals merge_reference over the two shards' order-matched oracle lists, bit for bit."""
    import merge_ref
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == 2
    import datetime
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
    mod = _pkg.load()
    from importlib import import_module
    dmod = import_module("approximate_spmv_topk_amd.distributed")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    k, n_queries, batch, min_score = 100, 11, 4, -1e30
    m = merge_ref.signed_matrix(mod)
    r0, r1 = [(0, 37), (37, 3000)][rank]
    shard = merge_ref.shard_of(mod, m, r0, r1)
    xs = np.stack([mod.create_sample_vector(m.cols, True, False, True, 700 + i) for i in range(n_queries)])
    dxs = torch.from_numpy(xs).to(dev)
    eng = mod.SpMV(shard.row, shard.col, shard.val, shard.rows, shard.cols, k=k, device=0, first_row=r0, min_score=min_score)
    step = dmod.NativeShardedSpMV(eng, dev, host_exchange=True)
    assert step.world == world
    step.set_batch(batch)
    step.run_many(dxs.data_ptr(), n_queries, n_queries)
    vb, ib = step.read_batch()  # the last batch: queries 8, 9, 10
    last_n = n_queries % batch
    # (every collective comes before the first assertion on results, so a failing rank never leaves the other one waiting)
    mine = []
    for q in range(n_queries - last_n, n_queries):
        y, present = merge_ref.shard_oracle_scores(mod, O, shard, xs[q], k, eng)
        mine.append(merge_ref.shard_oracle_list(O, y, present, k, min_score, r0))
    both = [None] * world
    dist.all_gather_object(both, mine)  # (each rank's oracle list depends on its own engine's partition hint)
    assert vb.shape[0] == last_n
    for j in range(last_n):
        lists = [both[r][j] for r in range(world)]
        assert lists[0][2] == 37 and lists[1][2] == k
        ei, ev = merge_ref.merge_reference([(w[0], w[1]) for w in lists], [w[2] for w in lists], k)
        assert np.array_equal(ib[j], ei) and np.array_equal(vb[j].view(np.uint32), ev.view(np.uint32)), \
            f"query {n_queries - last_n + j}: merged list differs from merge_reference over the shards' oracle lists"
    v, i = step.read()
    assert np.array_equal(i, ib[-1]) and np.array_equal(v.view(np.uint32), vb[-1].view(np.uint32))
    step.close()
    eng.close()
    dist.barrier()
    dist.destroy_process_group()
    print("REHEARSAL_OK", rank)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "short-shards":
        main_short_shards()
    else:
        main()
