// kernels/row_vectors.hpp -- row_vectors_kernel: stored rows as dense query vectors (tkspmv_enqueue_row_vectors).
// Part of engine.hip (one translation unit: included there behind the other kernel headers; device code only).
#pragma once
#include <cstddef>
#include "common.hpp"
#include "../row_lookup.hpp"

namespace tkspmv {

// One wave (a workgroup of 64 threads) serves one requested row: locate, expand, accumulate.
//   locate      the shared lookup of row_lookup.hpp over pkt_row and part_first: wave-uniform bisection steps through the scalar
//               cache, then one to three looks at a packet's column words (every lane decodes its own C slots, the row ends are
//               counted with ballots).
//   expand      the dense vector is built in LDS -- zeros, then the row's values at their columns -- and written out coalesced
//               behind a barrier: the zero fill and the scatter come from different lanes and hit the same addresses, and two
//               plain stores to one global address are not ordered by the program alone.
//   accumulate  a column that occurs several times in the row contributes the fp32 sum of its entries in stream order,
//               starting from +0.0f. Every entry sets its column's bit in a bitmap with an LDS atomic; one that finds the bit
//               set marks the column as repeated. Entries of unmarked columns are stored with one plain LDS store each (all
//               lanes at once: the common case pays two bitmap accesses per entry); the entries of marked columns are added
//               lane by lane, slot by slot -- LDS executes a wave's instructions in order, so that is stream order.
// Reads stream copy 0 and the side tables; writes xs and len only. No engine state.
struct RowVecParams {
    const uint8_t *packets;
    const uint32_t *pkt_row, *part_first, *part_count;
    uint32_t n_packets, n_parts, packet_bytes;
    uint32_t cols, rows, first_row;
    const uint32_t *ids;  // [count] global row ids (first_row + local)
    float *xs;            // [count][cols]
    uint32_t *len;        // [count] entries of the row; 0xFFFFFFFF: id outside [first_row, first_row + rows); NULL: not wanted
};

template <int XCOLS>
struct RowVecLds {
    alignas(16) float x[XCOLS];  // (read back as float4 for the coalesced write)
    uint32_t seen[XCOLS / 32];      // columns that have an entry so far
    uint32_t repeated[XCOLS / 32];  // ... more than one
};

// The wave's view of the stream for locate_row (row_lookup.hpp). Holds scalars, not the parameter block: a block whose
// address is taken ends up in scratch memory.
template <int C, bool C12>
struct WaveRowView {
    const uint8_t *packets;
    const uint32_t *pkt_row_, *part_first_, *part_count_;
    uint32_t packet_bytes, lane;
    static constexpr uint32_t PE = 64u * (uint32_t)C;
    __device__ __forceinline__ uint32_t pkt_row(uint32_t p) const { return scalar_load(pkt_row_ + p); }
    __device__ __forceinline__ uint32_t part_first(uint32_t q) const { return scalar_load(part_first_ + q); }
    __device__ __forceinline__ uint32_t part_count(uint32_t q) const { return scalar_load(part_count_ + q); }
    __device__ __forceinline__ const uint8_t *packet(uint32_t p) const { return packets + (size_t)p * packet_bytes; }
    // bit j: this lane's slot lane * C + j ends a row
    __device__ __forceinline__ uint32_t lane_ends(uint32_t p) const {
        const uint8_t *pkt = packet(p);
        uint32_t e = 0u;
#pragma unroll
        for (int j = 0; j < C; ++j) e |= (uint32_t)(f32_colword_at(pkt, PE, (uint32_t)C, C12, lane * (uint32_t)C + (uint32_t)j) & COLW_ROW_END) << j;
        return e;
    }
    // row ends in the lanes below this one
    __device__ __forceinline__ uint32_t ends_below(uint32_t e) const {
        uint32_t below = 0u;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uint64_t b = __ballot((e >> j) & 1u);
            below += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        }
        return below;
    }
    __device__ __forceinline__ bool kth_end(uint32_t p, uint32_t k, uint32_t &slot) const {
        const uint32_t e = lane_ends(p);
        uint32_t n = ends_below(e), s = 0u;
        bool mine = false;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            n += (e >> j) & 1u;
            if (((e >> j) & 1u) && n == k) {
                s = lane * (uint32_t)C + (uint32_t)j;
                mine = true;
            }
        }
        const uint64_t who = __ballot(mine);  // (one lane at most)
        if (who == 0ull) return false;
        slot = __builtin_amdgcn_readfirstlane(__shfl(s, (int)__builtin_ctzll(who)));
        return true;
    }
    __device__ __forceinline__ bool last_end(uint32_t p, uint32_t &slot) const {
        const uint32_t e = lane_ends(p);
        const uint64_t who = __ballot(e != 0u);
        if (who == 0ull) return false;
        const uint32_t s = lane * (uint32_t)C + (31u - (uint32_t)__builtin_clz(e | 1u));
        slot = __builtin_amdgcn_readfirstlane(__shfl(s, 63 - (int)__builtin_clzll(who)));
        return true;
    }
};

template <int C, int XCOLS, bool C12>
__global__ void __launch_bounds__(64) row_vectors_kernel(const RowVecParams R) {
    static_assert((C == 4 || C == 8) && (!C12 || (C == 4 && XCOLS == 1024)), "row_vectors_kernel: fp32 packet streams of 4 or 8 entries per lane");
    constexpr uint32_t PE = 64u * (uint32_t)C;
    __shared__ RowVecLds<XCOLS> L;
    const uint32_t lane = threadIdx.x;
    const uint32_t id = scalar_load(R.ids + blockIdx.x);
    const uint32_t r = id - R.first_row;
    const bool in_range = id >= R.first_row && r < R.rows;
    const uint32_t cols = R.cols;  // (<= XCOLS: the engine picks the instantiation)

    for (uint32_t c = lane; c < cols; c += 64u) L.x[c] = 0.0f;
    for (uint32_t w = lane; w < (cols + 31u) / 32u; w += 64u) {
        L.seen[w] = 0u;
        L.repeated[w] = 0u;
    }

    const WaveRowView<C, C12> V{R.packets, R.pkt_row, R.part_first, R.part_count, R.packet_bytes, lane};
    RowRun run{0u, 0u, 0u, 0u};
    uint32_t n = 0u;
    if (in_range && locate_row(V, r, R.n_packets, R.n_parts, PE, run))
        n = row_run_entries(run, PE, f32_colword_at(V.packet(run.first_pkt), PE, (uint32_t)C, C12, run.first_slot));
    __syncthreads();  // the zeros are in place

    if (n != 0u) {
        for (uint32_t p = run.first_pkt; p <= run.last_pkt; ++p) {  // (wave-uniform)
            const uint8_t *pkt = V.packet(p);
            uint32_t col[C], bit[C];
            float v[C];
            bool in[C], rep[C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const uint32_t ss = lane * (uint32_t)C + (uint32_t)j;
                in[j] = (p > run.first_pkt || ss >= run.first_slot) && (p < run.last_pkt || ss <= run.last_slot);
                col[j] = ((uint32_t)f32_colword_at(pkt, PE, (uint32_t)C, C12, ss) >> COLW_COL_SHIFT) & (uint32_t)(XCOLS - 1);
                bit[j] = 1u << (col[j] & 31u);
                v[j] = f32_value_at(pkt, (uint32_t)C, ss);
            }
#pragma unroll
            for (int j = 0; j < C; ++j)
                if (in[j] && (atomicOr(&L.seen[col[j] >> 5], bit[j]) & bit[j])) atomicOr(&L.repeated[col[j] >> 5], bit[j]);
            __syncthreads();  // every repeated column of the row so far is marked
            bool any = false;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                rep[j] = in[j] && (L.repeated[col[j] >> 5] & bit[j]);
                any = any || rep[j];
                if (in[j] && !rep[j]) L.x[col[j]] = 0.0f + v[j];  // (the sum that starts from +0.0f: -0.0f comes out as +0.0f)
            }
            // the rare part, in stream order: lanes in turn, each lane its slots in turn
            for (uint64_t turn = __ballot(any); turn != 0ull; turn &= turn - 1ull) {
                if (lane == (uint32_t)__builtin_ctzll(turn)) {
#pragma unroll
                    for (int j = 0; j < C; ++j)
                        if (rep[j]) L.x[col[j]] = L.x[col[j]] + v[j];
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();

    float *out = R.xs + (size_t)blockIdx.x * cols;
    if ((cols & 3u) == 0u && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {
        for (uint32_t c = lane * 4u; c < cols; c += 256u) *reinterpret_cast<float4 *>(out + c) = *reinterpret_cast<const float4 *>(&L.x[c]);
    } else {
        for (uint32_t c = lane; c < cols; c += 64u) out[c] = L.x[c];
    }
    if (R.len != nullptr && lane == 0u) R.len[blockIdx.x] = in_range ? n : 0xFFFFFFFFu;
}

}  // namespace tkspmv
