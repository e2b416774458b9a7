// kernels/group_select.hpp -- Grouped top-k: the reduction from rows to groups (group_best_kernel, group_split_kernel) and the group
// ids of a result (group_ids_kernel). Part of engine.hip (one translation unit: included there only; device code only).
#pragma once
#include "radix_select.hpp"

namespace tkspmv {
namespace grouped_kernels {

// ------------------------------------------------------------------------------------------------------------
// Every row carries a label < n_groups; a query returns the k best GROUPS, each by its best eligible row (the row of the group that
// comes first in the result order: score descending, row descending). The SpMV-only variant of the stream kernel writes every row's
// score; group_best_kernel folds rows into d_gkey[label] = max over the group's eligible rows of (order key << 32 | row) -- the very
// key the selection ranks by, so the maximum IS the representative and does not depend on the order the rows arrive in --;
// group_split_kernel turns the keys into a score array over the groups and a group -> row table and zeroes the keys for the next
// query; the radix passes and the selection kernel then run over the groups as they run over rows (pos_to_row = the table).
// ------------------------------------------------------------------------------------------------------------
struct GroupParams {
    const float *scores;       // [rows]; -inf: the row has no entry or is masked
    const uint32_t *groups;    // [rows] labels < n_groups
    unsigned long long *gkey;  // [n_groups]; 0 between queries
    float *gscore;             // [n_groups] the representative's score, -inf for a group without one
    uint32_t *grow;            // [n_groups] the representative's local row
    uint32_t *n_nonempty;      // groups that have a representative (zeroed in front of the query)
    uint32_t rows, n_groups;
    uint32_t kmin;             // order key of min_score: keys below it are not eligible
};
constexpr uint32_t GROUP_THREADS = 256;
constexpr uint32_t GROUP_LANE_ROWS = 4;  // consecutive rows per lane: 16 bytes of scores and 16 bytes of labels, one load each
constexpr uint32_t GROUP_TILE = 64u * GROUP_LANE_ROWS;  // rows a wave reduces at a time
constexpr uint32_t NO_GROUP = 0xFFFFFFFFu;  // label of the slots beyond the last row (n_groups is a uint32: no label reaches it), group id of a pad

// One run's maximum goes to its group's word; the result is not used (a no-return atomic). v = 0: the run holds no eligible row.
__device__ __forceinline__ void group_offer(unsigned long long *gkey, uint32_t label, unsigned long long v) {
    if (v != 0ull) (void)__hip_atomic_fetch_max(&gkey[label], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long group_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// Lane <-> four consecutive rows, lane by lane consecutive: a wave reads a tile of 256 rows with one 16-byte load of scores and one of
// labels per lane (both arrays are the engine's own allocations and a lane starts at a multiple of four rows, so the loads are
// aligned; the lane that holds the matrix' last rows loads them one by one). Adjacent rows with the same label form a run (a
// document's passages are stored together). Inside a lane the four rows are folded serially: a run that begins and ends inside the
// lane is offered at once; the lane keeps the maximum H of the run that holds its first row and T of the run that holds its last
// (H = T = the lane's maximum when all four labels agree). Across the lanes an inclusive segmented max over T -- six steps of
// shuffles, run heads where a lane holds a run boundary or its first label differs from the last label of the lane below -- leaves
// each run's maximum in the lane where the run ends, which alone offers it; a lane with a boundary also closes the run that
// entered it, H joined with what the lane below carried. Contiguous groups: one atomic per run and tile. Scattered labels: every
// row is a run of its own, one atomic per eligible row, which is correct, just slower.
__global__ void __launch_bounds__(GROUP_THREADS) group_best_kernel(const GroupParams G) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * GROUP_THREADS + threadIdx.x) >> 6, n_waves = gridDim.x * (GROUP_THREADS / 64u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)G.rows + GROUP_TILE - 1u) / GROUP_TILE);
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {  // wave-uniform
        const uint64_t r0 = (uint64_t)t * GROUP_TILE + lane * GROUP_LANE_ROWS;  // (64 bits: the last tile may reach past 2^32)
        float sc[GROUP_LANE_ROWS];
        uint32_t lab[GROUP_LANE_ROWS];
        if (r0 + GROUP_LANE_ROWS <= (uint64_t)G.rows) {
            const float4 s4 = *reinterpret_cast<const float4 *>(G.scores + r0);
            const uint4 g4 = *reinterpret_cast<const uint4 *>(G.groups + r0);
            sc[0] = s4.x, sc[1] = s4.y, sc[2] = s4.z, sc[3] = s4.w;
            lab[0] = g4.x, lab[1] = g4.y, lab[2] = g4.z, lab[3] = g4.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < GROUP_LANE_ROWS; ++j) {
                const bool in = r0 + j < (uint64_t)G.rows;
                sc[j] = in ? G.scores[r0 + j] : -__builtin_huge_valf();
                lab[j] = in ? G.groups[r0 + j] : NO_GROUP;
            }
        }
        unsigned long long c[GROUP_LANE_ROWS];
#pragma unroll
        for (uint32_t j = 0; j < GROUP_LANE_ROWS; ++j) {
            const uint32_t key = order_key(sc[j]);
            // (a slot beyond the last row holds -inf: never eligible; an eligible row's id fits 32 bits)
            c[j] = (sc[j] > -__builtin_huge_valf() && key >= G.kmin) ? (((unsigned long long)key << 32) | (uint32_t)(r0 + j)) : 0ull;
        }
        // inside the lane
        const bool b01 = lab[0] != lab[1], b12 = lab[1] != lab[2], b23 = lab[2] != lab[3];
        const bool split = b01 || b12 || b23;
        unsigned long long H = c[0], T = c[3];
        if (!b01) H = group_max(H, c[1]);
        if (!b01 && !b12) H = group_max(H, c[2]);
        if (!b23) T = group_max(T, c[2]);
        if (!b23 && !b12) T = group_max(T, c[1]);
        if (!split) H = T = group_max(H, T);
        if (b01 && b12) group_offer(G.gkey, lab[1], c[1]);                                 // row 1 alone
        if (b12 && b23) group_offer(G.gkey, lab[2], c[2]);                                 // row 2 alone
        if (b01 && !b12 && b23) group_offer(G.gkey, lab[1], group_max(c[1], c[2]));         // rows 1 and 2
        // across the lanes
        const uint32_t below = (uint32_t)__shfl_up((int)lab[3], 1), above = (uint32_t)__shfl_down((int)lab[0], 1);
        const bool joins = lane != 0u && below == lab[0];  // the run of this lane's first row began in a lane below
        bool head = split || !joins;
        unsigned long long v = T;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long ov = __shfl_up(v, d);
            const bool oh = __shfl_up((int)head, d) != 0;
            if (lane >= d) {
                if (!head) v = group_max(v, ov);
                head = head || oh;
            }
        }
        const unsigned long long carried = __shfl_up(v, 1);  // what the lane below holds for the run of its last row
        // (a non-zero maximum means the run holds an eligible row, so its label is a real one, < n_groups by tkspmv_set_groups' check)
        if (split) group_offer(G.gkey, lab[0], joins ? group_max(H, carried) : H);
        if (lane == 63u || above != lab[3]) group_offer(G.gkey, lab[3], v);
    }
}

// One thread per group: the key's two halves go where the selection reads them, the key itself back to 0.
__global__ void __launch_bounds__(GROUP_THREADS) group_split_kernel(const GroupParams G) {
    const uint32_t g = blockIdx.x * GROUP_THREADS + threadIdx.x;
    const bool in = g < G.n_groups;
    const unsigned long long key = in ? G.gkey[g] : 0ull;
    if (in) {
        G.gscore[g] = key != 0ull ? key_to_float((uint32_t)(key >> 32)) : -__builtin_huge_valf();
        G.grow[g] = (uint32_t)key;
        if (key != 0ull) G.gkey[g] = 0ull;
    }
    const uint64_t bm = __ballot(key != 0ull);
    if ((threadIdx.x & 63u) == 0u && bm) atomicAdd(G.n_nonempty, (uint32_t)__popcll(bm));
}

// The group ids of one result list: grp[i] = groups[idx[i] - first_row] for the n = min(k, non-empty groups) real entries, NO_GROUP for
// the pads behind them.
struct GroupIdsParams {
    const uint32_t *idx;         // [k] the selection's row ids (global)
    const uint32_t *groups;      // [rows]
    const uint32_t *n_nonempty;
    uint32_t *grp;               // [k]
    uint32_t *n_out;             // one word
    uint32_t k, rows, first_row;
};
__global__ void __launch_bounds__(GROUP_THREADS) group_ids_kernel(const GroupIdsParams P) {
    const uint32_t i = blockIdx.x * GROUP_THREADS + threadIdx.x;
    const uint32_t found = *P.n_nonempty, n = found < P.k ? found : P.k;
    if (i == 0u) *P.n_out = n;
    if (i >= P.k) return;
    const uint32_t r = P.idx[i] - P.first_row;
    P.grp[i] = (i < n && r < P.rows) ? P.groups[r] : NO_GROUP;
}

}  // namespace grouped_kernels
}  // namespace tkspmv
