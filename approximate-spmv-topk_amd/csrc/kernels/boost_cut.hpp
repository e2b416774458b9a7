// kernels/boost_cut.hpp -- Boosted top-k: the per-row transform of a query's scores fused with the cut at the cursor
// (boost_cut_kernel). Part of engine.hip (one translation unit: included there only; device code only).
#pragma once
#include "after_select.hpp"

namespace tkspmv {
namespace boost_kernels {

using after_kernels::AfterCursor;
using after_kernels::AfterParams;
using after_kernels::CURSOR_AFTER;
using after_kernels::CURSOR_START;

// ------------------------------------------------------------------------------------------------------------
// A boost is a per-row transform of the score array of the search-after path: with s the score the SpMV-only kernel wrote,
//     t = weight ? weight[r] * s : s,   s' = bias ? t + bias[r] : t      (two separately rounded fp32 operations, never an fma)
// and everything behind it -- eligibility, the order, the cut at the cursor, the count -- reads s'. A slot that holds -inf (a row
// without entries, a masked row) stays -inf whatever weight and bias say (0 * -inf is NaN: the test comes first), and an s' that is
// not finite becomes -inf: neither is ever eligible. The radix passes read the array behind this kernel, so s' goes to memory --
// in the same pass that cuts and counts, with ONE predicated 4-byte store per row, and none where the slot holds the final
// value already (weight 1, bias -0.0, a product or a sum that rounds to s).
// ------------------------------------------------------------------------------------------------------------
struct BoostParams {
    AfterParams A;        // the cut's own parameters, as after_cut_kernel takes them
    const float *weight;  // [rows] by LOCAL row, or NULL: no multiply
    const float *bias;    // [rows] by LOCAL row, or NULL: no add
    uint32_t wide;        // both arrays (where given) start at a multiple of 16 bytes: a lane's four rows are one load each
};
constexpr uint32_t BOOST_THREADS = 256;
constexpr uint32_t BOOST_LANE_ROWS = 4;  // consecutive rows per lane: 16 bytes of scores, one load
constexpr uint32_t BOOST_TILE = 64u * BOOST_LANE_ROWS;  // rows a wave takes at a time

__device__ __forceinline__ float boosted_score(float s, float w, float b, bool has_w, bool has_b) {
    if (s == -__builtin_huge_valf()) return s;
    float t = has_w ? __fmul_rn(w, s) : s;
    if (has_b) t = __fadd_rn(t, b);
    return __builtin_fabsf(t) < __builtin_huge_valf() ? t : -__builtin_huge_valf();  // (NaN compares false)
}

// after_cut_kernel's geometry: lane <-> four consecutive rows, 16-byte loads of the scores (the engine's own allocation) and, when
// the host found the caller's arrays aligned (BoostParams::wide), of weight and bias too; the lane that holds the matrix' last rows
// loads one by one, and so does every lane for arrays that are not aligned. The cursor's three words are the same for every lane.
__global__ void __launch_bounds__(BOOST_THREADS) boost_cut_kernel(const BoostParams B) {
    const AfterParams &A = B.A;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * BOOST_THREADS + threadIdx.x) >> 6, n_waves = gridDim.x * (BOOST_THREADS / 64u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)A.rows + BOOST_TILE - 1u) / BOOST_TILE);
    const bool has_w = B.weight != nullptr, has_b = B.bias != nullptr, wide = B.wide != 0u;
    uint32_t state = CURSOR_START;
    unsigned long long ceiling = 0ull;  // a row is behind the cursor when its key is BELOW this (END: 0, no key is)
    if (A.cursor) {
        state = A.cursor->state;
        if (state == CURSOR_AFTER) ceiling = ((unsigned long long)order_key(__uint_as_float(A.cursor->score_bits)) << 32) | A.cursor->row;
    }
    const bool from_top = state == CURSOR_START;
    uint32_t left = 0u;  // eligible rows behind the cursor this wave has seen (wave-uniform)
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {  // wave-uniform
        const uint64_t r0 = (uint64_t)t * BOOST_TILE + lane * BOOST_LANE_ROWS;  // (64 bits: the last tile may reach past 2^32)
        float sc[BOOST_LANE_ROWS], w[BOOST_LANE_ROWS], b[BOOST_LANE_ROWS];
        const bool full = r0 + BOOST_LANE_ROWS <= (uint64_t)A.rows;
        if (full) {
            const float4 s4 = *reinterpret_cast<const float4 *>(A.y + r0);
            sc[0] = s4.x, sc[1] = s4.y, sc[2] = s4.z, sc[3] = s4.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) sc[j] = r0 + j < (uint64_t)A.rows ? A.y[r0 + j] : -__builtin_huge_valf();
        }
        if (full && wide) {
            const float4 w4 = has_w ? *reinterpret_cast<const float4 *>(B.weight + r0) : float4{1.0f, 1.0f, 1.0f, 1.0f};
            const float4 b4 = has_b ? *reinterpret_cast<const float4 *>(B.bias + r0) : float4{0.0f, 0.0f, 0.0f, 0.0f};
            w[0] = w4.x, w[1] = w4.y, w[2] = w4.z, w[3] = w4.w;
            b[0] = b4.x, b[1] = b4.y, b[2] = b4.z, b[3] = b4.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) {
                const bool in = r0 + j < (uint64_t)A.rows;
                w[j] = has_w && in ? B.weight[r0 + j] : 1.0f;
                b[j] = has_b && in ? B.bias[r0 + j] : 0.0f;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) {
            // (a slot beyond the last row holds -inf: it stays -inf, and is neither stored to nor counted)
            const float v = boosted_score(sc[j], w[j], b[j], has_w, has_b);
            const uint32_t key = order_key(v);
            const bool real = v > -__builtin_huge_valf();
            const bool behind = from_top || ((((unsigned long long)key << 32) | (uint32_t)(A.first_row + (uint32_t)(r0 + j))) < ceiling);
            const float out = real && !behind ? -__builtin_huge_valf() : v;
            if (__float_as_uint(out) != __float_as_uint(sc[j])) A.y[r0 + j] = out;
            left += (uint32_t)__popcll(__ballot(real && behind && key >= A.kmin));
        }
    }
    if (lane == 0u && left != 0u) (void)__hip_atomic_fetch_add(A.total, left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace boost_kernels
}  // namespace tkspmv
