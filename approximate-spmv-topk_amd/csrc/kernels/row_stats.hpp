// kernels/row_stats.hpp -- row_stats_kernel: one statistic of every stored row (tkspmv_enqueue_row_stats): its entry count, its L1
// norm, the square of its L2 norm, or the cosine weight 1 / L2.
// Part of engine.hip (one translation unit: included there behind the other kernel headers; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"

namespace tkspmv {

// The scan kernels' loop (range_kernel is the template) with nothing around it: no x, no LDS, no candidate list, no threshold, no
// atomics, no timetable, and no workgroup ever waits for another. A row's statistic is the row's score with every product v * x[col]
// replaced by a function f(v) of the entry's own value:
//   ROW_NNZ    f = 1.0f            (exact below 2^24 entries per row)
//   ROW_L1     f = |v|
//   ROW_L2SQ   f = __fmul_rn(v, v)
//   ROW_INV_L2 L2SQ's sums, finished per row by inv_l2_of
// and the sums are reduce_core's, the function every streaming kernel calls: in-lane segmented sums, the clipped scan over the 64 lanes,
// the packet carry, +0.0f at a partition's start. So a statistic has the bits the streaming kernels would report for a query that makes
// every product f(v) -- which is what pins it to the order-matched oracle.
// Per packet: f of the lane's C values (the fp32 words as loaded: both fp32 layouts keep them whole), the row-end masks out of
// packet_flags -- the flag word range_kernel's expand path decodes --, reduce_core, expand, and one plain store per valid row end. Every
// row with entries is written exactly once, by the lane that holds its last entry; placeholders of empty rows and rows without packets
// are not written: the engine zeroes out[0 .. rows) in front of the launch, on the same stream.
// Reads stream copy 0 and pkt_row; writes out only. No engine state.
constexpr int ROW_STAT_NNZ = 0, ROW_STAT_L1 = 1, ROW_STAT_L2SQ = 2, ROW_STAT_INV_L2 = 3;

struct RowStatsParams {
    const uint8_t *packets;  // stream copy 0
    float *out;              // [rows], indexed by local row
    uint32_t rows;
};

// The cosine weight of a row whose squares sum to l2sq: two separately rounded IEEE operations, subnormals kept; +0.0f where the sum
// is 0, +inf or NaN, so every weight is finite (the largest: 1 / sqrt(2^-149) < 2^75). Spelled as the language's own sqrt and
// division, which hipcc rounds correctly by default: the header's __fsqrt_rn is the hardware's approximation (one ulp off for
// some arguments) unless OCML_BASIC_ROUNDED_OPERATIONS is defined, and the host restatements (packed_host.cpp, host.inv_l2) are IEEE.
__device__ __forceinline__ float inv_l2_of(float l2sq) {
    const float w = 1.0f / __builtin_sqrtf(l2sq);
    return (l2sq > 0.0f && l2sq < __builtin_huge_valf()) ? w : 0.0f;
}

// m[j] = all ones where bit j of the flag word is set (entry j ends a row): one bit-field extraction each.
template <int C, int J = 0>
__device__ __forceinline__ void row_end_masks(uint32_t fl, uint32_t (&m)[C]) {
    m[J] = bit_mask<J>(fl);
    if constexpr (J + 1 < C) row_end_masks<C, J + 1>(fl, m);
}

template <int C, bool C12, int KIND>
__global__ void __launch_bounds__(512, 4) row_stats_kernel(const StreamParams P, const RowStatsParams R) {
    static_assert((C == 4 || C == 8) && (!C12 || C == 4), "row_stats_kernel: fp32 packet streams of 4 or 8 entries per lane");
    static_assert(KIND >= ROW_STAT_NNZ && KIND <= ROW_STAT_INV_L2, "row_stats_kernel: four kinds");
    constexpr int QM = C12 ? QM_F32C12 : QM_F32;
    constexpr int VT = value_type_of(QM);
    constexpr bool BUF = C == 4;           // buffer loads (load_packet_buf) where they exist
    constexpr int NBUF = C == 8 ? 2 : 3;   // range_kernel's packet buffers
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bid = blockIdx.x, n_wg = gridDim.x;
    const uint32_t total_waves = (blockDim.x >> 6) * n_wg;
    const uint32_t part0 = wave * n_wg + bid;

    Pkt<C, VT> buf[NBUF];
    LaneOffsets lo{0u, 0u};
    if constexpr (BUF) lo = lane_offsets<C, VT>(lane);
    const uint8_t *pk = R.packets;
    __amdgpu_buffer_rsrc_t rsrc = stream_resource(pk, 0u);
    uint32_t req_off = 0u;

    for (uint32_t part = part0; part < P.n_parts; part += total_waves) {
        uint32_t f0 = 0u, n = 0u;
        TKSPMV_PARTITION_RANGE(P, part, f0, n);
        // (wave-uniform by construction; said so, or every packet offset becomes a vector value and each buffer load a loop over its lanes)
        f0 = __builtin_amdgcn_readfirstlane(f0);
        n = __builtin_amdgcn_readfirstlane(n);
        // The first NBUF - 1 packets of the partition (clamped to its last packet; a partition without packets has a resource of 0
        // bytes, whose loads return 0 and touch nothing).
        pk = R.packets + (size_t)f0 * P.packet_bytes;
        if constexpr (BUF) rsrc = stream_resource(pk, n * P.packet_bytes);
#pragma unroll
        for (int u = 0; u < NBUF - 1; ++u) {
            const uint32_t iu = ((uint32_t)u < n) ? (uint32_t)u : (n > 0u ? n - 1u : 0u);
            if constexpr (BUF) load_packet_buf<C, VT>(rsrc, iu * P.packet_bytes, lo, buf[u]);
            else if (n > 0u) load_packet<C, VT>(pk + (size_t)iu * P.packet_bytes, lane, buf[u]);
        }
        req_off = (n > (uint32_t)(NBUF - 1) ? (uint32_t)(NBUF - 1) : (n > 0u ? n - 1u : 0u)) * P.packet_bytes;  // the next request's packet
        float carry = 0.0f;  // (a partition starts on a row boundary)
        // NBUF - 1 packets in flight behind the one being reduced; the buffers rotate by NAME (the loop is unrolled by NBUF).
        for (uint32_t i0 = 0; i0 < n; i0 += NBUF) {
#pragma unroll
            for (int u = 0; u < NBUF; ++u) {
                const uint32_t i = i0 + (uint32_t)u;
                if (i >= n) break;
                const Pkt<C, VT> &cur = buf[u];
                // Unconditional (offset clamped to the last packet): a fixed number of younger loads lets the compiler wait with a
                // counted vmcnt instead of vmcnt(0).
                if constexpr (BUF) load_packet_buf<C, VT>(rsrc, req_off, lo, buf[(u + NBUF - 1) % NBUF]);
                else load_packet<C, VT>(pk + req_off, lane, buf[(u + NBUF - 1) % NBUF]);
                if (i + (uint32_t)NBUF < n) req_off += P.packet_bytes;
                const uint32_t rb = scalar_load(P.pkt_row + f0 + i);  // first row of the packet (scalar cache: retires through lgkmcnt)

                const uint32_t fl = packet_flags<C, QM>(cur);
                float p[C];
                uint32_t m[C];
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const float v = cur.v[j];
                    p[j] = KIND == ROW_STAT_NNZ ? 1.0f : (KIND == ROW_STAT_L1 ? __builtin_fabsf(v) : __fmul_rn(v, v));
                }
                row_end_masks<C>(fl, m);
                const Reduced<C> Rd = reduce_core<C, false>(p, m, (fl & ((1u << C) - 1u)) != 0u, carry);
                const RowSums<C> S = expand<C, false>(Rd, fl);
                uint32_t r = rb + ends_below<C>(S);
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    // (r < rows always holds for a stream the packers wrote; the comparison keeps a damaged table from writing outside out)
                    if (S.valid(j) && r < R.rows) R.out[r] = KIND == ROW_STAT_INV_L2 ? inv_l2_of(S.rs[j]) : S.rs[j];
                    r += S.end(j) ? 1u : 0u;
                }
            }
        }
    }
}

}  // namespace tkspmv
