"""A plain numpy reference of the shard merge (tkspmv_merge_topk*, distributed.merge_candidates) and the table of cases the
CPU and GPU tests run through it. Shares no code with the package: keys are uint64, the number of real entries of every
list is an INPUT (known by construction, or counted by the oracle's selection), never derived from the lists, so the
filler-suffix rule of the implementations is itself under test. Test infrastructure only."""
import numpy as np

NEG_ZERO = np.array([0x80000000], np.uint32).view(np.float32)[0]
SUBNORMAL = np.array([0x00000001], np.uint32).view(np.float32)[0]
NEG_SUBNORMAL = np.array([0x80000001], np.uint32).view(np.float32)[0]


def _keys(idx, val):
    """(order key of the score) << 32 | row id, as uint64: larger key = earlier in the merged list."""
    bits = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32).astype(np.uint64)
    neg = (bits >> np.uint64(31)) != 0
    okey = np.where(neg, bits ^ np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))
    return (okey << np.uint64(32)) | np.ascontiguousarray(idx, dtype=np.uint32).astype(np.uint64)


def merge_reference(lists, n_real, k):
    """lists: per shard (idx uint32[k], val float32[k]); n_real: per shard, how many leading entries are real.
    Returns (idx uint32[k], val float32[k]): every real entry of every shard by (score key desc, row id desc as unsigned),
    cut at k, padded with (0, +0.0f)."""
    idx = np.concatenate([np.asarray(i, dtype=np.uint32)[:n] for (i, _), n in zip(lists, n_real)] + [np.zeros(0, np.uint32)])
    val = np.concatenate([np.asarray(v, dtype=np.float32)[:n] for (_, v), n in zip(lists, n_real)] + [np.zeros(0, np.float32)])
    order = np.argsort(_keys(idx, val), kind="stable")[::-1][:k]  # (equal keys are equal entries: their order cannot show)
    out_idx = np.zeros(k, np.uint32)
    out_val = np.zeros(k, np.float32)
    out_idx[:order.shape[0]] = idx[order]
    out_val[:order.shape[0]] = val[order]
    return out_idx, out_val


def _case(name, k, shards):
    """shards: per shard the real entries [(row, score), ...] in the order given (tkspmv_read order unless the case says
    otherwise); every list is completed to k entries with fillers (0, +0.0f)."""
    world = len(shards)
    idx = np.zeros((world, k), np.uint32)
    val = np.zeros((world, k), np.float32)
    for r, entries in enumerate(shards):
        assert len(entries) <= k
        for j, (row, score) in enumerate(entries):
            idx[r, j] = row
            val[r, j] = score
    return {"name": name, "world": world, "k": k, "idx": idx, "val": val, "n_real": [len(e) for e in shards]}


def _read_order(entries):
    idx = np.array([e[0] for e in entries], np.uint32)
    val = np.array([e[1] for e in entries], np.float32)
    order = np.argsort(_keys(idx, val), kind="stable")[::-1]
    return [(int(idx[i]), val[i]) for i in order]


# Scores the random cases draw from: few values, so that equal score bits meet across shards and at the k-th boundary.
_PALETTE = np.array([-3.5, -1.0, -0.5, -0.25, -1e-3, NEG_SUBNORMAL, NEG_ZERO, 0.0, SUBNORMAL, 1e-3, 0.25, 0.5, 1.0, 7.0], np.float32)


def random_case(world, k, seed, first_rows=None):
    """Signed scores with many ties; shard r owns rows [first_row_r, first_row_r + 4k) and returns between 0 and k of them
    (now and then exactly 0 or k). Row 0 never scores +0.0f: that entry cannot be told from a filler (include/tkspmv.h)."""
    rng = np.random.RandomState(seed)
    shards = []
    for r in range(world):
        first = (r * 4 * k + 1) if first_rows is None else first_rows[r]
        n = int(rng.choice([0, k, rng.randint(0, k + 1), rng.randint(0, k + 1)]))
        rows = (np.uint64(first) + rng.permutation(4 * k)[:n].astype(np.uint64)).astype(np.uint32)
        half = rng.rand(n) < 0.5
        scores = np.where(half, rng.choice(_PALETTE, n), (rng.rand(n) - 0.5).astype(np.float32)).astype(np.float32)
        scores[(rows == 0) & (scores.view(np.uint32) == 0)] = np.float32(0.125)
        shards.append(_read_order(list(zip(rows.tolist(), scores))))
    return _case(f"random_w{world}_k{k}_s{seed}", k, shards)


EXAMPLE_A = [(3, -0.1), (1, -0.4)]
EXAMPLE_B = [(17, 0.5), (12, -0.2), (15, -0.3), (11, -0.5)]


def table():
    """The hand-made cases and one random case per (world, k) of the CPU table."""
    t = [
        _case("example_k4", 4, [EXAMPLE_A, EXAMPLE_B]),
        _case("example_k8", 8, [EXAMPLE_A, EXAMPLE_B]),
        _case("all_fillers", 5, [[], [], []]),
        _case("fewer_than_k", 6, [[(4, 0.5), (2, -0.5)], [(30, -0.25)], [(61, 0.75), (60, -2.0)]]),
        _case("exactly_k", 6, [[(4, 0.5), (2, -0.5), (1, -0.75)], [(30, -0.25)], [(61, 0.75), (60, -2.0)]]),
        _case("k_plus_one", 6, [[(4, 0.5), (2, -0.5), (1, -0.75)], [(30, -0.25), (31, -3.0)], [(61, 0.75), (60, -2.0)]]),
        # equal score bits in two shards at the k-th boundary: the larger row id wins, as unsigned 32-bit
        _case("tie_at_kth", 3, [[(10, 0.9), (5, 0.25)], [(20, 0.8), (9, 0.25)]]),
        _case("tie_at_kth_negative", 3, [[(10, -0.1), (5, -0.25)], [(20, -0.2), (9, -0.25)]]),
        _case("tie_at_kth_unsigned_ids", 3, [[(10, 0.9), (5, 0.25)], [(0x80000001, 0.8), (0x80000000, 0.25)]]),
        # (0, -0.0f) is a real entry: last before the fillers, last of a full list, and (not in read order) behind negatives
        _case("neg_zero_row0_then_fillers", 4, [[(5, 1.0), (0, NEG_ZERO)], [(9, -0.5), (8, -1.0), (7, -2.0)]]),
        _case("neg_zero_row0_ends_full_list", 2, [[(5, 1.0), (0, NEG_ZERO)], [(9, -0.5), (8, -1.0)]]),
        _case("neg_zero_row0_behind_negatives", 6, [[(3, -0.5), (2, -0.75), (0, NEG_ZERO)], [(9, -0.25), (8, -1.0)]]),
        # (r > 0, +0.0f) is a real entry: it outranks the negative scores, the fillers behind it do not
        _case("pos_zero_real_rows", 5, [[(9, 0.5), (6, 0.0), (2, 0.0)], [(40, -0.25), (41, -0.5)]]),
        _case("pos_zero_real_row_ends_list", 3, [[(9, 0.5), (6, 0.0), (2, 0.0)], [(40, -0.25), (41, -0.5)]]),
        _case("subnormals", 4, [[(0, SUBNORMAL), (3, NEG_SUBNORMAL)], [(12, 0.0), (11, NEG_ZERO), (10, -1e-38)]]),
        _case("rows_at_and_above_2_31", 4, [[(0x80000000, 0.5), (0x7FFFFFFF, 0.5), (0x80000001, -0.5)],
                                            [(0xFFFFF000, 0.5), (0xFFFFFFFF, -0.5), (0xFFFFF003, -0.5)]]),
    ]
    for world, k in ((1, 1), (2, 1), (5, 1), (3, 7), (8, 100)):
        t.append(random_case(world, k, seed=11 * world + k))
    t.append(random_case(3, 7, seed=99, first_rows=[1, 0x7FFFFFF0, 0xFFFFF000]))
    return t


def lists_of(case):
    return [(case["idx"][r], case["val"][r]) for r in range(case["world"])]


def expected(case):
    return merge_reference(lists_of(case), case["n_real"], case["k"])


def gathered(cases):
    """The [world][n_q][2][k] int32 buffer an all-gather leaves behind, query q holding cases[q] (same world and k)."""
    world, k = cases[0]["world"], cases[0]["k"]
    g = np.zeros((world, len(cases), 2, k), np.int32)
    for q, c in enumerate(cases):
        assert (c["world"], c["k"]) == (world, k)
        g[:, q, 0, :] = c["idx"].view(np.int32)
        g[:, q, 1, :] = c["val"].view(np.int32)
    return g


# ---- real shard engines: the signed matrix, its shards and each shard's order-matched oracle list ---------------------
def signed_matrix(pkg, rows=3000, cols=128, per_row=8, seed=3):
    """rows x cols, per_row entries in every row, values uniform in [-0.5, 0.5): scores of both signs (the shape of
    test_gpu_engine.py::test_negative_scores_and_min_score). The same bytes in every process that builds it."""
    rng = np.random.RandomState(seed)
    col = np.sort(rng.randint(0, cols, (rows, per_row)), axis=1).astype(np.uint32).reshape(-1)
    val = (rng.rand(rows * per_row).astype(np.float32) - np.float32(0.5)).astype(np.float32)
    row = np.repeat(np.arange(rows, dtype=np.uint32), per_row)
    return pkg.CooMatrix(rows, cols, row, col, val)


def shard_of(pkg, m, r0, r1):
    lo, hi = np.searchsorted(m.row, r0, side="left"), np.searchsorted(m.row, r1, side="left")
    return pkg.CooMatrix(r1 - r0, m.cols, (m.row[lo:hi] - np.uint32(r0)).astype(np.uint32), m.col[lo:hi], m.val[lo:hi])


def shard_oracle_scores(pkg, oracle, shard, x, k, eng):
    """(scores float32[rows], present uint8[rows]) of a shard in the order its engine sums them: the shard packed again with
    the host packer and the engine's partition hint, scored by the oracle's model of the streaming kernels."""
    info = eng.info()
    C = info["packet_entries"] // 64
    packed = pkg.Packed(shard, k=k, nnz_per_lane=C, n_wave_partitions=(info["batch_mode"] >> 16) or info["n_wave_partitions"])
    assert packed.info()["n_wave_partitions"] == info["n_wave_partitions"]
    return oracle.packed_scores(packed.raw(), x, shard.rows, C)


def shard_oracle_list(oracle, y, present, k, min_score, first_row):
    """(idx, val, n_real): what the shard's engine must return, and how many of its entries the selection found eligible."""
    idx, val = oracle.select_topk(y, present, k, min_score, first_row)
    n_real = min(k, int(np.count_nonzero((present != 0) & (y >= np.float32(min_score)))))
    return idx, val, n_real
