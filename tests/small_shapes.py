"""Short label runs and tiny matrices: what test_small_shapes_host.py and test_gpu_small_shapes.py share. A plain module like
support.py and dense_ends.py (no fixtures, no hooks).

A. Short label runs, for group_best_kernel (kernels/group_select.hpp). A lane of that kernel holds 4 consecutive rows of a 256-row
   tile. What it does with them depends on the three in-lane label boundaries b01, b12, b23, on whether the run of its first row
   began in the lane below (joins; never in lane 0) and on whether the run of its last row goes on in the lane above (continues;
   never in lane 63 nor in the lane of the matrix' last row): 32 situations. run_matrix(rows) has one entry per row over RUN_COLS
   columns, its values a seeded permutation of 1 .. rows, so with a query of ones (times a power of two) every score is an exact,
   distinct integer in any summation order: the expectation is run_scores(), no oracle. run_labels(rows) draws run lengths from
   RUN_LENGTHS and gives run i the label i % N_GROUPS: neighbouring runs differ, most groups own two or more separate runs (the
   atomic maximum across runs), and N_GROUPS <= the engines' k = RUN_K, so every group's representative is in the result.

   Measured with seed = row count (run_labels: default_rng(rows); run_matrix: default_rng([rows, 1])), pooled over RUN_ROWS =
   6001 .. 6004 (rows % 4 = 1, 2, 3, 0) (coverage() of lane_situations(); asserted by test_small_shapes_host.py):
     1. each of the 32 (b01, b12, b23, joins, continues) occurs at least 4 times: the rarest occurs 6 times;
     2. for each of them and each of the 4 in-lane positions some lane has its row at that position as the best row of its run:
        128 of 128 pairs;
     3. runs that span a 256-row tile boundary: 17, 19, 16 and 14 in the four matrices, the run's best row in front of the boundary
        in 8, 10, 8 and 8 of them and behind it in 9, 9, 8 and 6.

B. Tiny matrices, for every call: TINY names 18 shapes by their row lengths -- one row; one row of 9; rows < 4 x 2; empty rows at
   the end and in front; one 700-entry row that spans packets between two empty rows; and 31 .. 1025 rows around the wave (64), the
   4-rows-per-lane kernels' tile (256) and the largest k (1024), their lengths cycling CYCLE. Signed values, seeded, columns
   sorted per row. tiny_ks() gives the three k of a shape's engines: 1, the rows with entries, rows + 47 (both capped at 1024)."""
import numpy as np

import support

# ---- A: short label runs ---------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 1, 2, 2, 3, 3, 4, 5, 7)
RUN_ROWS = (6001, 6002, 6003, 6004)        # rows % 4 = 1, 2, 3, 0
RUN_C8 = 6003                              # the row count that also runs at 8 entries per lane
RUN_COLS, N_GROUPS, RUN_K = 64, 900, 1024
TILE, LANE_ROWS = 256, 4                   # group_best_kernel's GROUP_TILE and GROUP_LANE_ROWS
NO_GROUP = 0xFFFFFFFF                      # what the kernel puts into the slots beyond the last row
LIFT = np.float32(1e6)                     # tile_bias(): above every score (<= 2 * 6004), and score + LIFT is exact below 2^24


def run_labels(rows, seed=None):
    """(labels uint32[rows], run int64[rows]): run lengths drawn from RUN_LENGTHS (seed: the row count), run i labelled
    i % N_GROUPS; the last run is cut at the matrix' end."""
    rng = np.random.default_rng(rows if seed is None else seed)
    ends = np.cumsum(rng.choice(RUN_LENGTHS, rows))
    run = np.searchsorted(ends, np.arange(rows), side="right")
    return (run % N_GROUPS).astype(np.uint32), run


def run_matrix(pkg, rows, seed=None):
    """rows x RUN_COLS with exactly one entry per row, the values a seeded permutation of 1 .. rows."""
    rng = np.random.default_rng([rows if seed is None else seed, 1])
    val = (rng.permutation(rows) + 1).astype(np.float32)
    return support.coo(pkg, rows, RUN_COLS, np.arange(rows), rng.integers(0, RUN_COLS, rows), val)


def run_scores(m, scale=1.0):
    """What row r scores for the query of RUN_COLS times `scale` (a power of two): exact in float32 in any order."""
    assert np.array_equal(m.row, np.arange(m.rows))
    return (m.val * np.float32(scale)).astype(np.float32)


def run_mask(rows, labels, run):
    """An allow-mask that removes about 30 % of the rows: whole runs (12 % of them), whole groups (label % 10 == 3: they end
    empty) and single rows (12 %), so that groups lose their best row."""
    rng = np.random.default_rng(rows + 7)
    drop_run = rng.random(int(run.max()) + 1) < 0.12
    return ~(drop_run[run] | (labels % 10 == 3) | (rng.random(rows) < 0.12))


def tile_bias(rows):
    """float32[rows]: LIFT on one seeded row of every 256-row tile, 0 elsewhere."""
    rng = np.random.default_rng(rows + 11)
    b = np.zeros(rows, dtype=np.float32)
    for t0 in range(0, rows, TILE):
        b[t0 + int(rng.integers(0, min(TILE, rows - t0)))] = LIFT
    return b


def lane_situations(labels, scores):
    """The lanes of group_best_kernel that hold at least one row, as the kernel sees them: [((b01, b12, b23, joins, continues),
    positions)] with positions the in-lane offsets 0 .. 3 whose row is the best-scoring row of its run (the run of adjacent equal
    labels in the whole matrix). The slots beyond the last row carry NO_GROUP."""
    rows = labels.size
    n_lanes = (rows + LANE_ROWS - 1) // LANE_ROWS
    lab = np.full((n_lanes + 1) * LANE_ROWS, NO_GROUP, dtype=np.int64)
    lab[:rows] = labels
    run = np.cumsum(np.concatenate([[0], labels[1:] != labels[:-1]]))
    best = np.zeros(lab.size, dtype=bool)
    order = np.lexsort((scores, run))  # by run, then by score: a run's last entry is its best row (the scores are distinct)
    best[order[np.concatenate([run[order][1:] != run[order][:-1], [True]])]] = True
    out = []
    for i in range(n_lanes):
        r0, lane = i * LANE_ROWS, i % (TILE // LANE_ROWS)
        l4 = lab[r0:r0 + LANE_ROWS]
        joins = lane != 0 and lab[r0 - 1] == l4[0]
        continues = lane != 63 and i != n_lanes - 1 and lab[r0 + LANE_ROWS] == l4[3]
        t = (bool(l4[0] != l4[1]), bool(l4[1] != l4[2]), bool(l4[2] != l4[3]), bool(joins), bool(continues))
        out.append((t, [p for p in range(LANE_ROWS) if best[r0 + p]]))
    return out


def tile_spans(labels, scores):
    """[(tile boundary, best row)] of the runs with rows on both sides of a multiple of TILE."""
    out = []
    for b in range(TILE, labels.size, TILE):
        if labels[b - 1] == labels[b]:
            lo, hi = b - 1, b
            while lo > 0 and labels[lo - 1] == labels[b]:
                lo -= 1
            while hi + 1 < labels.size and labels[hi + 1] == labels[b]:
                hi += 1
            out.append((b, lo + int(np.argmax(scores[lo:hi + 1]))))
    return out


def coverage(pkg, row_counts=RUN_ROWS):
    """(occurrences of each tuple, the (tuple, position) pairs reached, [spans per matrix]) pooled over the row counts."""
    seen, pairs, spans = {}, set(), []
    for rows in row_counts:
        labels, _ = run_labels(rows)
        y = run_scores(run_matrix(pkg, rows))
        for t, pos in lane_situations(labels, y):
            seen[t] = seen.get(t, 0) + 1
            pairs.update((t, p) for p in pos)
        spans.append(tile_spans(labels, y))
    return seen, pairs, spans


# ---- B: tiny matrices --------------------------------------------------------------------------------------------------------------
CYCLE = (3, 0, 1, 7, 2)
CYCLE_ROWS = (31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
TINY = {"one_row": ([1], 8), "one_row_of_9": ([9], 32), "rows_2_3_4": ([2, 3, 4], 16), "empty_tail": ([4, 4, 4, 0, 0, 0], 16),
        "empty_front": ([0, 0, 0, 5, 1], 16), "long_row": ([0, 700, 0], 1024)}
TINY.update({f"rows{r}": ([CYCLE[i % len(CYCLE)] for i in range(r)], 64) for r in CYCLE_ROWS})
C8_ROWS = (1, 33, 257, 1025)      # the shapes whose engines are also made with 8 entries per lane
FIRST_ROW_ROWS = (33, 257)        # the shapes with one more engine at first_row = FIRST_ROW
FIRST_ROW = 5000
MAX_K = 1024


def tiny(pkg, name):
    """The COO of TINY[name]: signed values without zeros, the columns of a row distinct and sorted."""
    ln, cols = TINY[name]
    ln = np.asarray(ln, dtype=np.int64)
    rng = np.random.default_rng(1000 + list(TINY).index(name))
    row = np.repeat(np.arange(ln.size), ln)
    col = np.concatenate([np.sort(rng.choice(cols, n, replace=False)) for n in ln if n]).astype(np.uint32)
    val = rng.standard_normal(row.size).astype(np.float32)
    val[val == 0] = np.float32(0.5)
    return support.coo(pkg, ln.size, cols, row, col, val)


def tiny_vectors(cols, count=3, seed=7):
    """Signed query vectors without zeros."""
    xs = np.random.default_rng([seed, cols]).standard_normal((count, cols)).astype(np.float32)
    xs[xs == 0] = np.float32(0.25)
    return xs


def tiny_ks(m):
    """The k of a shape's three engines: 1, the rows with entries, rows + 47 -- both at most MAX_K --, each once."""
    n = int(support.present(m).sum())
    return list(dict.fromkeys([1, min(MAX_K, n), min(MAX_K, m.rows + 47)]))


def tiny_engines(m):
    """[(entries per lane, k, first_row, multi_q)] of a shape's engines: the three k at 4 entries per lane, and at 8 for C8_ROWS; one
    at first_row = FIRST_ROW for FIRST_ROW_ROWS; and one created with multi_q = 2 for enqueue_multi."""
    ks = tiny_ks(m)
    specs = [(4, k, 0, 0) for k in ks]
    if m.rows in C8_ROWS:
        specs += [(8, k, 0, 0) for k in ks]
    if m.rows in FIRST_ROW_ROWS:
        specs.append((4, ks[1], FIRST_ROW, 0))
    specs.append((4, ks[1], 0, 2))
    return specs


def tiny_masks(rows):
    """The four allow-masks of the filtered call: every row, none, exactly the last row, the odd rows."""
    r = np.arange(rows)
    return {"all": np.ones(rows, dtype=bool), "none": np.zeros(rows, dtype=bool), "last_row": r == rows - 1, "odd_rows": r % 2 == 1}


def tiny_labelings(rows):
    """name -> (labels uint32[rows], n_groups) of the grouped calls."""
    r = np.arange(rows)
    return {"thirds": ((r // 3).astype(np.uint32), (rows + 2) // 3), "mod2": ((r % 2).astype(np.uint32), 2), "identity": (r.astype(np.uint32), rows)}
