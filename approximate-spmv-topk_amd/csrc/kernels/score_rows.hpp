// kernels/score_rows.hpp -- score_rows_kernel: the scores of GIVEN rows for given queries (tkspmv_enqueue_score_rows), from the
// rows' own packets: no pass over the matrix.
// Part of engine.hip (one translation unit: included there behind row_vectors.hpp; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"
#include "row_vectors.hpp"

namespace tkspmv {

// One wave serves one list entry: locate the row (row_lookup.hpp, through row_vectors.hpp's WaveRowView), then for every query of
// the item run the row's packets through reduce_core -- the arithmetic of every streaming kernel -- with
//   * the carry +0.0f in front of the row's first packet, carried across the row's packets;
//   * every slot's own ROW_END mask;
//   * the products of the slots outside the row replaced by +0.0f: x is gathered (from global memory: it is small, read by every
//     wave and stays in the L2) for the row's slots only.
// The clipped scan never lets a value cross a row end, and the carry that enters a packet whose slot 0 starts a row is +0.0f in
// the full stream too, so the sum at the row's end slot has the bits the streaming kernels report.
// An item is a list entry i and a chunk of q_per_item queries: with one list for every query (ids_stride = 0) the row is located
// once for the whole chunk; with a list per query the engine sets q_per_item = 1. One item per wave, no loop over items: with such
// a loop around it the kernel needed more scalar registers than there are.
// Reads stream copy 0 and the side tables; writes scores only. No engine state.
struct ScoreRowsParams {
    const uint8_t *packets;
    const uint32_t *pkt_row, *part_first, *part_count;
    uint32_t n_packets, n_parts, packet_bytes;
    uint32_t cols, rows, first_row;
    const float *xs;       // [n_q][cols]
    const uint32_t *ids;   // query q's list: ids + q * ids_stride, n_rows global row ids (first_row + local)
    float *scores;         // [n_q][n_rows]
    uint64_t ids_stride;   // 0: one list for every query
    uint32_t n_q, n_rows;
    uint32_t q_per_item;   // queries per item: workgroup (x, y) serves list entries 4 x .. 4 x + 3 for queries y * q_per_item ...
};

constexpr uint32_t SCORE_ROWS_WAVES = 4;  // waves per workgroup: the lookup is a chain of dependent loads, hidden by occupancy

// A lane's share of a packet: its C column words and values (plain loads: a row's packets are read once per query of the item).
template <int C>
struct RowPkt {
    uint32_t w[C];
    float v[C];
};
template <int C, bool C12>
__device__ __forceinline__ RowPkt<C> load_row_packet(const uint8_t *pkt, uint32_t lane) {
    constexpr uint32_t PE = 64u * (uint32_t)C;
    RowPkt<C> k;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t ss = lane * (uint32_t)C + (uint32_t)j;
        k.w[j] = f32_colword_at(pkt, PE, (uint32_t)C, C12, ss);
        k.v[j] = f32_value_at(pkt, (uint32_t)C, ss);
    }
    return k;
}
// bit j: the lane's slot lane * C + j of packet p belongs to the run
template <int C>
__device__ __forceinline__ uint32_t slots_inside(const RowRun &run, uint32_t p, uint32_t lane) {
    uint32_t in = 0u;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const uint32_t ss = lane * (uint32_t)C + (uint32_t)j;
        in |= (uint32_t)((p > run.first_pkt || ss >= run.first_slot) && (p < run.last_pkt || ss <= run.last_slot)) << j;
    }
    return in;
}
// One packet of the row for one query: products inside the run, +0.0f outside, then the shared reduction.
template <int C>
__device__ __forceinline__ Reduced<C> reduce_row_packet(const RowPkt<C> &k, uint32_t inside, const float *xq, float &carry) {
    float p[C];
    uint32_t m[C];
    uint32_t any = 0u;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        p[j] = 0.0f;
        if ((inside >> j) & 1u) p[j] = __fmul_rn(k.v[j], xq[k.w[j] >> COLW_COL_SHIFT]);
        m[j] = bit_mask<0>(k.w[j]);
        any |= k.w[j];
    }
    return reduce_core<C, false>(p, m, (any & (uint32_t)COLW_ROW_END) != 0u, carry);
}
// The row sum at stream slot `slot` (wave-uniform; a row end) of the packet just reduced, in every lane.
template <int C>
__device__ __forceinline__ float row_sum_at(const Reduced<C> &R, uint32_t slot) {
    const RowSums<C> sums = expand<C, false>(R, 0u);
    const uint32_t j = slot % (uint32_t)C;
    float s = sums.rs[0];
#pragma unroll
    for (int t = 1; t < C; ++t) s = j == (uint32_t)t ? sums.rs[t] : s;
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), (int)(slot / (uint32_t)C)));
}

template <int C, bool C12>
__global__ void __launch_bounds__(64 * SCORE_ROWS_WAVES) score_rows_kernel(const ScoreRowsParams S) {
    static_assert((C == 4 || C == 8) && (!C12 || C == 4), "score_rows_kernel: fp32 packet streams of 4 or 8 entries per lane");
    constexpr uint32_t PE = 64u * (uint32_t)C;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const WaveRowView<C, C12> V{S.packets, S.pkt_row, S.part_first, S.part_count, S.packet_bytes, lane};
    const uint32_t cols = S.cols, n_rows = S.n_rows;

    // (every loop and branch below is wave-uniform: reduce_core moves values across all 64 lanes)
    // One item per wave, no loop over items: the grid covers them (the engine cuts what exceeds a grid into several launches).
    const uint32_t i = blockIdx.x * SCORE_ROWS_WAVES + wave;
    if (i >= n_rows) return;
    const uint32_t q0 = blockIdx.y * S.q_per_item;
    const uint32_t nq = S.n_q - q0 < S.q_per_item ? S.n_q - q0 : S.q_per_item;
    const uint32_t id = scalar_load(S.ids + (size_t)q0 * S.ids_stride + i);
    const uint32_t r = id - S.first_row;
    const bool in_range = id >= S.first_row && r < S.rows;
    float *out = S.scores + (size_t)q0 * n_rows + i;  // query q0 + t: out[t * n_rows]
    const float *xq = S.xs + (size_t)q0 * cols;       // ... and xq + t * cols
    RowRun run{0u, 0u, 0u, 0u};
    bool has_entries = false;
    if (in_range && locate_row(V, r, S.n_packets, S.n_parts, PE, run)) {
        run.first_pkt = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.first_pkt);
        run.first_slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.first_slot);
        run.last_pkt = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.last_pkt);
        run.last_slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.last_slot);
        has_entries = !(f32_colword_at(V.packet(run.first_pkt), PE, (uint32_t)C, C12, run.first_slot) & COLW_SKIP);
    }
    if (!has_entries) {  // a placeholder or no packets at all: +0.0f, as tkspmv_scores reports it; an id outside: -inf
        const float s = in_range ? 0.0f : -__builtin_huge_valf();
#pragma unroll 1
        for (uint32_t t = lane; t < nq; t += 64u) out[(size_t)t * n_rows] = s;
        return;
    }
    if (run.last_pkt - run.first_pkt <= 1u) {
        // the common case, one or two packets: decoded once, kept in registers across the queries
        const bool two = run.last_pkt != run.first_pkt;
        const RowPkt<C> a = load_row_packet<C, C12>(V.packet(run.first_pkt), lane);
        const RowPkt<C> b = load_row_packet<C, C12>(V.packet(run.last_pkt), lane);
        const uint32_t in_a = slots_inside<C>(run, run.first_pkt, lane), in_b = slots_inside<C>(run, run.last_pkt, lane);
#pragma unroll 1
        for (uint32_t t = 0; t < nq; ++t, xq += cols, out += n_rows) {
            float carry = 0.0f;
            Reduced<C> R = reduce_row_packet<C>(a, in_a, xq, carry);
            if (two) R = reduce_row_packet<C>(b, in_b, xq, carry);
            const float s = row_sum_at<C>(R, run.last_slot);
            if (lane == 0u) *out = s;
        }
    } else {
        // a long row: its packets are read again for every query (from the caches)
#pragma unroll 1
        for (uint32_t t = 0; t < nq; ++t, xq += cols, out += n_rows) {
            float carry = 0.0f;
            Reduced<C> R{};
#pragma unroll 1
            for (uint32_t p = run.first_pkt; p <= run.last_pkt; ++p) {
                const RowPkt<C> k = load_row_packet<C, C12>(V.packet(p), lane);
                R = reduce_row_packet<C>(k, slots_inside<C>(run, p, lane), xq, carry);
            }
            const float s = row_sum_at<C>(R, run.last_slot);
            if (lane == 0u) *out = s;
        }
    }
}

}  // namespace tkspmv
