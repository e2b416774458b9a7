// kernels/after_select.hpp -- Search-after paging: the cut at the cursor (after_cut_kernel) and the page's bookkeeping
// (after_finish_kernel). Part of engine.hip (one translation unit: included there only; device code only).
#pragma once
#include "radix_select.hpp"

namespace tkspmv {
namespace after_kernels {

// ------------------------------------------------------------------------------------------------------------
// The result order is a strict total order -- (order key << 32 | global row id), descending: make_ckey's key with the global id --,
// so "every eligible row strictly behind entry (row, score)" is a set, and the k first of it are the next page. The SpMV-only variant
// of the stream kernel writes every row's score; after_cut_kernel replaces the score of every row that does NOT rank behind the
// query's cursor by -inf (never eligible) and counts the eligible rows that remain; the radix passes and the selection kernel then
// run over the scores as they do for a large k; after_finish_kernel turns the count and the list's last real entry into n, the
// hits left and the cursor of the following page. A cursor is a position in the order, nothing more: it need not name a row.
// ------------------------------------------------------------------------------------------------------------
struct AfterCursor {  // tkspmv_cursor (include/tkspmv.h) as the device reads and writes it
    uint32_t row, score_bits, state, reserved;
};
constexpr uint32_t CURSOR_START = 0u, CURSOR_AFTER = 1u, CURSOR_END = 2u;  // (any other state acts as END)

struct AfterParams {
    float *y;                   // [rows] the query's scores; -inf: the row has no entry or is masked
    const AfterCursor *cursor;  // this query's cursor in device memory (NULL: START)
    uint32_t *total;            // += eligible rows behind the cursor (zero in front of the query)
    uint32_t rows, first_row;
    uint32_t kmin;              // order key of min_score: keys below it are not eligible
};
constexpr uint32_t AFTER_THREADS = 256;
constexpr uint32_t AFTER_LANE_ROWS = 4;  // consecutive rows per lane: 16 bytes of scores, one load
constexpr uint32_t AFTER_TILE = 64u * AFTER_LANE_ROWS;  // rows a wave cuts at a time

// Lane <-> four consecutive rows as in group_best_kernel (y is the engine's own allocation and a lane starts at a multiple of four
// rows, so the 16-byte load is aligned; the lane that holds the matrix' last rows loads them one by one). The cursor's three words
// are the same for every lane. A row that is not behind the cursor gets -inf with a predicated 4-byte store (a row that holds -inf
// already gets none): on a shallow page almost no lane stores; END stores everywhere, which is slow, correct and rare.
__global__ void __launch_bounds__(AFTER_THREADS) after_cut_kernel(const AfterParams A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * AFTER_THREADS + threadIdx.x) >> 6, n_waves = gridDim.x * (AFTER_THREADS / 64u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)A.rows + AFTER_TILE - 1u) / AFTER_TILE);
    uint32_t state = CURSOR_START;
    unsigned long long ceiling = 0ull;  // a row is behind the cursor when its key is BELOW this (END: 0, no key is)
    if (A.cursor) {
        state = A.cursor->state;
        if (state == CURSOR_AFTER) ceiling = ((unsigned long long)order_key(__uint_as_float(A.cursor->score_bits)) << 32) | A.cursor->row;
    }
    const bool from_top = state == CURSOR_START;
    uint32_t left = 0u;  // eligible rows behind the cursor this wave has seen (wave-uniform)
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {  // wave-uniform
        const uint64_t r0 = (uint64_t)t * AFTER_TILE + lane * AFTER_LANE_ROWS;  // (64 bits: the last tile may reach past 2^32)
        float sc[AFTER_LANE_ROWS];
        if (r0 + AFTER_LANE_ROWS <= (uint64_t)A.rows) {
            const float4 s4 = *reinterpret_cast<const float4 *>(A.y + r0);
            sc[0] = s4.x, sc[1] = s4.y, sc[2] = s4.z, sc[3] = s4.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < AFTER_LANE_ROWS; ++j) sc[j] = r0 + j < (uint64_t)A.rows ? A.y[r0 + j] : -__builtin_huge_valf();
        }
#pragma unroll
        for (uint32_t j = 0; j < AFTER_LANE_ROWS; ++j) {
            const uint32_t key = order_key(sc[j]);
            // (a slot beyond the last row holds -inf: neither stored to nor counted)
            const bool real = sc[j] > -__builtin_huge_valf();
            const bool behind = from_top || ((((unsigned long long)key << 32) | (uint32_t)(A.first_row + (uint32_t)(r0 + j))) < ceiling);
            if (real && !behind) A.y[r0 + j] = -__builtin_huge_valf();
            left += (uint32_t)__popcll(__ballot(real && behind && key >= A.kmin));
        }
    }
    if (lane == 0u && left != 0u) (void)__hip_atomic_fetch_add(A.total, left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Behind the selection: n = min(k, total), the hits left, and the cursor of the following page -- AFTER(the last real entry) when
// rows remain behind this page, END otherwise (so a loop "while state != END" ends without an empty trailing page). The count word
// goes back to 0 for the next query. next may be the cursor this query read: the cut has finished in stream order.
struct AfterFinishParams {
    const uint32_t *idx;  // [k] the selection's list (global row ids)
    const float *val;
    uint32_t *total;      // the count word of after_cut_kernel
    uint32_t *n_out, *total_out;  // one word each, or NULL
    AfterCursor *next;    // or NULL
    uint32_t k;
};
constexpr uint32_t AFTER_FINISH_THREADS = 64;
__global__ void __launch_bounds__(AFTER_FINISH_THREADS) after_finish_kernel(const AfterFinishParams P) {
    if (threadIdx.x != 0u) return;
    const uint32_t total = *P.total, n = total < P.k ? total : P.k;
    if (P.n_out) *P.n_out = n;
    if (P.total_out) *P.total_out = total;
    if (P.next) {
        AfterCursor c{0u, 0u, CURSOR_END, 0u};
        if (total > P.k) {  // (k >= 1: n - 1 names the list's last entry)
            c.row = P.idx[n - 1u];
            c.score_bits = __float_as_uint(P.val[n - 1u]);
            c.state = CURSOR_AFTER;
        }
        *P.next = c;
    }
    *P.total = 0u;
}

}  // namespace after_kernels
}  // namespace tkspmv
