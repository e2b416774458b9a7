"""Hand-built matrices whose packets end many rows, and the allow-masks that go with them: what test_mask_window_host.py and
test_gpu_mask_window.py share. A plain module like support.py (no fixtures, no hooks).

The allow-mask readers (mask_pair / mask_rows in kernels/packet_math.hpp, mask_entries in kernels/col_stats.hpp) prefetch two mask
words per packet and fetch further words only for a packet whose rows reach past them: 33 .. 64 row ends or more in one packet. The
generated matrices of the other tests (about 13 row ends per packet) never get there. matrix() does, in every packet of its first
sections; test_mask_window_host.py asserts that from the packed stream.

The section lengths are not round numbers: they were chosen so that, for every row count of ROWS, both variants and 4 and 8 entries
per lane, some packet starts at a row == 31 mod 32, and so that in a stream of PREPACKED_PARTITIONS partitions the first ordinary row
opens a mask word (ORDINARY % 32 == 0), begins in the last slots of a packet that ends more than two mask words of one-entry rows
(at a multiple of 512 slots minus 14) and goes on in the next packet: the one case in which mask_entries needs a word that mask_rows
does not.

tkspmv_create refuses none of the sizes of TINY_ROWS."""
import numpy as np

import support

COLS = 1024
ONES, EMPTY, SMALL, AFTER_LONG = 640, 307, 226, 490  # rows per section, in the order of matrix()'s docstring
LONG = 700                                           # entries of the long row
FULL = COLS - 1                                      # entries of a full last row: every column but one (1024 entries would fill their packets to the last slot and leave the last partition without padding)
LONG_ROW = ONES + EMPTY + SMALL                      # its index
ORDINARY = LONG_ROW + 1 + AFTER_LONG                 # the first ordinary row
MIN_ORDINARY = 1000                                  # enough packets of ordinary rows for every start residue the properties ask for
ROWS = (2687, 2688, 2689)                            # the smallest with rows % 32 in {0, 1, 31} that hold every section
VARIANTS = ("last_empty", "last_full")
TINY_ROWS = (1, 31, 32, 33, 64, 65)
DENSE_LAST = (255, 511)                              # the last row the first packet ends at 4 and at 8 entries per lane
PREPACKED_PARTITIONS = 2                             # Packed(..., n_wave_partitions=) of the prepacked engines: partitions of many packets


def lengths(rows, variant):
    """The row lengths of matrix(rows, variant)."""
    assert variant in VARIANTS and rows >= ORDINARY + MIN_ORDINARY + 1, (rows, variant)
    small = np.random.default_rng(1504).integers(0, 4, SMALL)  # (the sections in front of the ordinary rows do not depend on rows)
    ordinary = np.random.default_rng(1).integers(1, 31, rows - ORDINARY - 1)
    last = 0 if variant == "last_empty" else FULL
    return np.concatenate([np.ones(ONES, dtype=np.int64), np.zeros(EMPTY, dtype=np.int64), small, [LONG], np.ones(AFTER_LONG, dtype=np.int64),
                           ordinary, [last]]).astype(np.int64)


def matrix(pkg, rows, variant):
    """A COO of `rows` rows over 1024 columns with signed values, laid out in this order: ONES rows of exactly one entry; EMPTY rows
    without entries (each is stored as a placeholder with a row end); SMALL rows of 0 .. 3 entries drawn at random; one row of 700
    entries followed immediately by AFTER_LONG one-entry rows -- packets without a row end next to packets that end hundreds --;
    ordinary rows of 1 .. 30 entries; a last row that is empty or full -- every column but one, FULL -- (variant)."""
    ln = lengths(rows, variant)
    assert ln.size == rows
    rng = np.random.default_rng(rows * 2 + VARIANTS.index(variant))
    row = np.repeat(np.arange(rows), ln)
    col = np.concatenate([np.sort(rng.choice(COLS, n, replace=False)) for n in ln if n]).astype(np.uint32)
    val = rng.standard_normal(row.size).astype(np.float32)
    val[val == 0] = np.float32(0.5)
    return support.coo(pkg, rows, COLS, row, col, val)


def packet_table(packed, m):
    """[(rb, n_ends, continues, padding)] per packet of a Packed, from raw()'s pkt_row and partition table: the packet's first row; the
    rows it ends; whether the row behind them has entries in this packet and goes on in the partition's next; and, for a partition's
    last packet, the slots the partition leaves unused (padding)."""
    _, _, pkt_row, part_first, part_count = packed.raw()
    pe = packed.info()["packet_entries"]
    slots = np.concatenate([[0], np.cumsum(np.maximum(np.bincount(m.row, minlength=m.rows), 1))])  # (an empty row takes one slot)
    out = []
    for p in range(part_first.size):
        f, n = int(part_first[p]), int(part_count[p])
        r_first = int(pkt_row[f])
        r_next = int(pkt_row[part_first[p + 1]]) if p + 1 < part_first.size else m.rows
        for i in range(n):
            rb = int(pkt_row[f + i])
            nxt = int(pkt_row[f + i + 1]) if i + 1 < n else r_next
            continues = i + 1 < n and int(slots[nxt] - slots[r_first]) < (i + 1) * pe
            out.append((rb, nxt - rb, continues, n * pe - int(slots[r_next] - slots[r_first]) if i + 1 == n else 0))
    return out


def tiny(pkg, rows):
    """rows in TINY_ROWS: a few entries per row, rows 0, 3, 6, .. empty (the one-row matrix's row 0 holds entries): rows 31, 32 and
    64, which open and close mask words, hold entries."""
    assert rows in TINY_ROWS
    rng = np.random.default_rng(100 + rows)
    ln = np.where((np.arange(rows) % 3 == 0) & (rows > 1), 0, rng.integers(1, 6, rows))
    row = np.repeat(np.arange(rows), ln)
    col = np.concatenate([np.sort(rng.choice(COLS, n, replace=False)) for n in ln if n]).astype(np.uint32)
    val = rng.standard_normal(row.size).astype(np.float32)
    val[val == 0] = np.float32(0.5)
    return support.coo(pkg, rows, COLS, row, col, val)


def vector(seed=7):
    """A signed query vector without zeros."""
    x = np.random.default_rng(seed).standard_normal(COLS).astype(np.float32)
    x[x == 0] = np.float32(0.25)
    return x


def _single(rows, r):
    a = np.zeros(rows, dtype=bool)
    a[r] = True
    return a


def masks(rows):
    """name -> bool[rows]. alt_words: the rows of even words allowed, those of odd words not (a wrong word pick flips every answer),
    and its complement; word_edges: bits 0 and 31 of every word; single rows at the word boundaries, at the last row, at the last
    row a dense packet ends, at the first row behind the long row and at the first ordinary row."""
    r = np.arange(rows)
    out = {"random50": np.random.default_rng(rows).random(rows) < 0.5,
           "alt_words": (r >> 5) % 2 == 0, "alt_words_inv": (r >> 5) % 2 == 1,
           "word_edges": (r % 32 == 0) | (r % 32 == 31),
           "none": np.zeros(rows, dtype=bool)}
    for name, i in (("row31", 31), ("row32", 32), ("row63", 63), ("row64", 64), ("last_row", rows - 1), ("dense_last_c4", DENSE_LAST[0]),
                    ("dense_last_c8", DENSE_LAST[1]), ("after_long", LONG_ROW + 1), ("first_ordinary", ORDINARY)):
        if i < rows:
            out[name] = _single(rows, i)
    return out


def tiny_masks(rows):
    """The alt-bit masks of the tiny matrices: even rows, odd rows."""
    r = np.arange(rows)
    return {"even_rows": r % 2 == 0, "odd_rows": r % 2 == 1}


def words(pkg, rows, allow, dirty):
    """row_mask(rows, allow); dirty: with every bit at and beyond `rows` set in the last word (the header says they are ignored)."""
    w = pkg.row_mask(rows, allow).copy()
    if dirty and rows % 32:
        w[-1] |= np.uint32((0xFFFFFFFF << (rows % 32)) & 0xFFFFFFFF)
    return w
