// kernels/label_sums.hpp -- label_sums_kernel: the column sums of the stored rows of every label, as 64-bit fixed-point integers
// (tkspmv_enqueue_label_sums), and label_sums_close_kernel, which turns them into floats (tkspmv_enqueue_sums_close).
// Part of engine.hip (one translation unit: included there behind col_stats.hpp; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"
#include "col_stats.hpp"  // load_stat_packet, column_offset
#include "row_stats.hpp"  // inv_l2_of
#include "../quantise.hpp"

namespace tkspmv {

// col_stats_kernel<..., EXT = true, FILT = true>'s launch, packet prefetch with counted waits, walk back to the partition's last row
// end and live / SKIP rule, over stream copy 0. Where that kernel tests the mask bit of an entry's row, this one loads the row's label:
// the row of the lane's entry j is rb + (row ends in lower lanes) + (row ends among the lane's entries 0 .. j-1) -- mask_entries'
// arithmetic --, at most C consecutive rows per lane and packet; an entry behind the packet's last row end belongs to the row that
// continues in the next packet and gets that row's label. The row index is clamped to rows - 1, so no load leaves the array; padding,
// whose row may lie beyond the partition's rows, is excluded by `live`, never by a label.
// Every counted entry (r, c, v) adds quantise(v, E) (quantise.hpp) to word [labels[r]][c]; a label >= n_bins has no bin. Two sinks:
//   LDS_SINK: uint64 bins [B][XCOLS], B = 8192 / XCOLS, in one static block of 64 KiB at LDS offset 0; one 64-bit LDS atomic per
//     counted entry whose label lies in the launch's window [b0, b0 + B); behind the workgroup's last partition the non-zero words
//     are swept to sums with 64-bit agent-scope atomics (col_stats_kernel's flush). More than B bins: one launch per window.
//   direct: one 64-bit agent-scope atomic per counted entry straight into sums[label][col]; no LDS, every bin in one launch.
// Integer add is associative and commutative: the sums do not depend on the geometry, the partition cuts or the order of the atomics.
// Reads stream copy 0, pkt_row and labels; adds to sums only. No engine state.
struct LabelSumsParams {
    const uint8_t *packets;    // stream copy 0
    const uint32_t *labels;    // [rows], indexed by local row
    unsigned long long *sums;  // [n_bins][cols] two's complement words, zeroed (or holding earlier sums) in front of the launch
    uint32_t rows;
    uint32_t n_bins;
    uint32_t b0;               // LDS_SINK: first bin of the launch's window
    int32_t quantum_exp;
};

constexpr uint32_t LABEL_SUMS_LDS_WORDS = 8192u;  // 64 KiB of 64-bit bins, whatever the tier
constexpr uint32_t label_sums_lds_bins(int xcols) { return xcols <= (int)LABEL_SUMS_LDS_WORDS ? LABEL_SUMS_LDS_WORDS / (uint32_t)xcols : 0u; }

typedef __attribute__((address_space(3))) unsigned long long lds_wu64;

template <int C, int XCOLS, bool C12, bool LDS_SINK>
__global__ void __launch_bounds__(512, 4) label_sums_kernel(const StreamParams P, const LabelSumsParams R) {
    static_assert((C == 4 || C == 8) && (!C12 || C == 4), "label_sums_kernel: fp32 packet streams of 4 or 8 entries per lane");
    static_assert(!LDS_SINK || (XCOLS <= (int)LABEL_SUMS_LDS_WORDS && LABEL_SUMS_LDS_WORDS % XCOLS == 0), "the LDS sink holds whole bins of XCOLS words");
    constexpr int QM = C12 ? QM_F32C12 : QM_F32;
    constexpr int VT = value_type_of(QM);
    constexpr int NBUF = C == 8 ? 2 : 3;  // whole packets: range_kernel's packet buffers
    constexpr uint32_t PE = 64u * (uint32_t)C;
    constexpr uint32_t B = LDS_SINK ? LABEL_SUMS_LDS_WORDS / (uint32_t)XCOLS : 1u;
    __shared__ unsigned long long bins[LDS_SINK ? LABEL_SUMS_LDS_WORDS : 1u];  // the kernel's only __shared__ block: LDS offset 0
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bid = blockIdx.x, n_wg = gridDim.x;
    const uint32_t total_waves = (blockDim.x >> 6) * n_wg;
    const uint32_t part0 = wave * n_wg + bid;
    const uint32_t coff = col_offset<C, VT>(lane);
    const uint32_t last_row = R.rows - 1u;  // (rows >= 1: the engine launches nothing otherwise)
    // bins of the launch's window that exist: a label outside [b0, b0 + window) deposits nothing (one unsigned comparison)
    const uint32_t window = LDS_SINK ? (R.n_bins - R.b0 < B ? R.n_bins - R.b0 : B) : R.n_bins;
    const uint32_t b0 = LDS_SINK ? R.b0 : 0u;
    uint32_t hbase = 0u;

    if constexpr (LDS_SINK) {
        hbase = lds_addr_of(bins);
        for (uint32_t w = tid; w < LABEL_SUMS_LDS_WORDS; w += 512u) bins[w] = 0ull;
        __syncthreads();
    }

    Pkt<C, VT> buf[NBUF];
    for (uint32_t part = part0; part < P.n_parts; part += total_waves) {
        uint32_t f0 = 0u, n_all = 0u;
        TKSPMV_PARTITION_RANGE(P, part, f0, n_all);
        // (wave-uniform by construction; said so, or every packet offset becomes a vector value: row_stats_kernel)
        f0 = __builtin_amdgcn_readfirstlane(f0);
        n_all = __builtin_amdgcn_readfirstlane(n_all);
        // The first NBUF - 1 packets (clamped to the partition's last packet; a partition without packets has a resource of 0 bytes,
        // whose loads return 0 and touch nothing).
        const __amdgpu_buffer_rsrc_t rsrc = stream_resource(R.packets + (size_t)f0 * P.packet_bytes, n_all * P.packet_bytes);
#pragma unroll
        for (int u = 0; u < NBUF - 1; ++u) {
            const uint32_t iu = ((uint32_t)u < n_all) ? (uint32_t)u : (n_all > 0u ? n_all - 1u : 0u);
            load_stat_packet<C, VT, true>(rsrc, iu * P.packet_bytes, lane, coff, buf[u]);
        }
        uint32_t req_off = (n_all > (uint32_t)(NBUF - 1) ? (uint32_t)(NBUF - 1) : (n_all > 0u ? n_all - 1u : 0u)) * P.packet_bytes;  // the next request's packet
        // The partition's last row end: packets [0, n) are visited, and in packet n - 1 the slots up to last_slot are counted.
        uint32_t n = 0u, last_slot = 0u;
        for (uint32_t p = n_all; p > 0u; --p) {
            Pkt<C, VT> tail;
            load_stat_packet<C, VT, false>(rsrc, (p - 1u) * P.packet_bytes, lane, coff, tail);
            const uint32_t ends = packet_flags<C, QM>(tail) & ((1u << C) - 1u);
            const uint64_t eb = __ballot(ends != 0u);
            if (eb != 0ull) {
                const uint32_t top = 63u - (uint32_t)__builtin_clzll(eb);
                const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ends, (int)top);
                n = p;
                last_slot = top * (uint32_t)C + (31u - (uint32_t)__builtin_clz(e));
                break;
            }
        }
        // NBUF - 1 packets in flight behind the one being summed; the buffers rotate by NAME (the loop is unrolled by NBUF).
        for (uint32_t i0 = 0; i0 < n; i0 += NBUF) {
#pragma unroll
            for (int u = 0; u < NBUF; ++u) {
                const uint32_t i = i0 + (uint32_t)u;
                if (i >= n) break;
                const Pkt<C, VT> &cur = buf[u];
                const uint32_t rb = scalar_load(P.pkt_row + f0 + i);  // first row of the packet

                // The labels of the lane's C entries, requested in FRONT of the next packet: the packet loads stay the youngest
                // requests, so the wait for the labels is a counted one too.
                const uint32_t fl = packet_flags<C, QM>(cur);
                const uint32_t ends = (uint32_t)__popc(fl & ((1u << C) - 1u));
                uint32_t below = 0u;
#pragma unroll
                for (int b = 0; (1 << b) <= C; ++b) {  // sum over the lower lanes of numbers of at most C, bit by bit (mask_entries)
                    const uint64_t eb = __ballot(((ends >> b) & 1u) != 0u);
                    below += __builtin_amdgcn_mbcnt_hi((uint32_t)(eb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)eb, 0u)) << b;
                }
                const uint32_t r0 = rb + below;  // the row of the lane's entry 0
                uint32_t lab[C];
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const uint32_t r = r0 + (uint32_t)__popc(fl & ((1u << j) - 1u));
                    lab[j] = R.labels[r < last_row ? r : last_row];
                }
                // Unconditional (offset clamped to the last packet): a fixed number of younger loads lets the compiler wait with a
                // counted vmcnt instead of vmcnt(0).
                load_stat_packet<C, VT, true>(rsrc, req_off, lane, coff, buf[(u + NBUF - 1) % NBUF]);
                if (i + (uint32_t)NBUF < n_all) req_off += P.packet_bytes;

                // slots of the lane that lie in front of the padding: entry j iff lane * C + j <= last_slot in the last packet
                const uint32_t lim = i + 1u == n ? last_slot : PE - 1u;
                const uint32_t lc = lane * (uint32_t)C;
                const uint32_t live = lim < lc ? 0u : (lim - lc >= (uint32_t)C - 1u ? (1u << C) - 1u : (2u << (lim - lc)) - 1u);
                const uint32_t counted = live & ~(fl >> 8);
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const uint32_t bin = lab[j] - b0;
                    if (((counted >> j) & 1u) && bin < window) {
                        const unsigned long long q = (unsigned long long)quantise(__float_as_uint(cur.v[j]), R.quantum_exp);
                        const uint32_t c4 = column_offset<C, XCOLS, QM>(cur, j);  // 4 * column, cut to the tier's width
                        if constexpr (LDS_SINK) {
                            lds_wu64 *const w = reinterpret_cast<lds_wu64 *>((uintptr_t)(hbase + bin * (uint32_t)XCOLS * 8u + c4 * 2u));
                            (void)__hip_atomic_fetch_add(w, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        } else if ((c4 >> 2) < P.cols) {  // (always, for a stream the packers wrote: keeps a damaged one inside sums)
                            (void)__hip_atomic_fetch_add(R.sums + (size_t)bin * P.cols + (c4 >> 2), q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                }
            }
        }
    }
    if constexpr (LDS_SINK) {
        // The workgroup's bins to global memory, non-zero words only (col_stats_kernel's flush).
        __syncthreads();
        for (uint32_t w = tid; w < LABEL_SUMS_LDS_WORDS; w += 512u) {
            const unsigned long long v = bins[w];
            const uint32_t bin = w / (uint32_t)XCOLS, c = w % (uint32_t)XCOLS;
            if (v != 0ull && bin < window && c < P.cols)
                (void)__hip_atomic_fetch_add(R.sums + (size_t)(b0 + bin) * P.cols + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Closing launch: one workgroup of 64 threads per bin. FLOAT: out[b][c] = ldexpf((float)sums[b][c], E), the conversion rounding to
// nearest even. UNIT: that value f_c times w = inv_l2_of((float)n2), n2 = the sum of (double)f_c * (double)f_c -- each product exact in
// double -- formed as 64 partials, lane l taking the columns l, l + 64, ... ascending, added by lane 0 in the order 0 .. 63: a fixed
// order, so the bits do not depend on anything. A bin with w == 0 (no entry, a zero sum, an overflowed norm) is NOT written. No atomics.
__global__ void __launch_bounds__(64) label_sums_close_kernel(const long long *sums, float *out, uint32_t cols, int32_t quantum_exp, uint32_t unit) {
    __shared__ double part[64];
    __shared__ float w_sh;
    const uint32_t lane = threadIdx.x;
    const long long *const s = sums + (size_t)blockIdx.x * cols;
    float *const o = out + (size_t)blockIdx.x * cols;
    if (!unit) {
        for (uint32_t c = lane; c < cols; c += 64u) o[c] = ldexpf((float)s[c], quantum_exp);
        return;
    }
    double acc = 0.0;
    for (uint32_t c = lane; c < cols; c += 64u) {
        const double f = (double)ldexpf((float)s[c], quantum_exp);
        acc += f * f;
    }
    part[lane] = acc;
    __syncthreads();
    if (lane == 0u) {
        double n2 = 0.0;
        for (int l = 0; l < 64; ++l) n2 += part[l];
        w_sh = inv_l2_of((float)n2);
    }
    __syncthreads();
    const float w = w_sh;
    if (w == 0.0f) return;
    for (uint32_t c = lane; c < cols; c += 64u) o[c] = __fmul_rn(ldexpf((float)s[c], quantum_exp), w);
}

}  // namespace tkspmv
