// kernels/assign.hpp -- assign_kernel: for every stored row the best-scoring of a set of vectors (tkspmv_enqueue_assign): the row's
// label (the vector's index) and its score against that vector.
// Part of engine.hip (one translation unit: included there behind row_stats.hpp; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"

namespace tkspmv {

// row_stats_kernel's loop (one pass over stream copy 0, one output per row, written by the lane that holds the row's last entry, no
// candidate list, no threshold, no atomics, no timetable, and no workgroup ever waits for another) with range_kernel's x in LDS --
// several of them: a launch serves up to QP = 16384 / XCOLS vectors (16 / 4 / 1), staged side by side in ONE static block of 64 KiB,
// copy q at byte offset q * 4 * XCOLS, a multiple of 4 KiB as reduce_packet's address rule ((word & 0xFFC) | base) requires. The block
// is the kernel's only __shared__ object, so it sits at LDS address 0; two workgroups fit a CU's 160 KiB.
// Staging is range_kernel's: clamped addresses, +0.0f beyond cols. (The wave-BSCSR streams have no padding slot with a value of its
// own inside x -- padding is +0.0 at column 0 --, so every word of the block has one writer and one value: the race DESIGN.md 3.7
// describes for the row-per-lane byte chunks has nothing to race about here.)
// Per packet and vector q of the launch: reduce_packet on copy q with the vector's OWN packet carry, then expand -- the calls, the
// order and hence the bits of every other streaming path --, and per row-end slot j a running pair (best, label): vector 0 sets it,
// a later one replaces it only where its sum is strictly greater (ties go to the smallest index). The loop over the vectors is
// unrolled at compile time (assign_vectors): the carries (wave-uniform, kept in vector registers between packets) and the pairs are
// named values, never a run-time-indexed array, which would live in scratch.
// Stores: one plain store per valid row end and output. The first launch of a call (q0 = 0) stores unconditionally; a later one, at
// vector offset q0, loads the row's stored best and replaces the pair only where its own best is strictly greater, its labels offset
// by q0. One lane of one wave of one launch touches a row, and the launches of a call follow each other in stream order, so the
// read-modify-write needs no atomics. Placeholders of empty rows and rows without packets are never written: the engine zeroes both
// outputs in front of the first launch, on the same stream (label 0, +0.0f).
// Reads stream copy 0 and pkt_row; writes labels and best only. No engine state.
struct AssignParams {
    const uint8_t *packets;  // stream copy 0
    const float *xs;         // vector i of the launch: xs + i * cols
    uint32_t *labels;        // [rows], indexed by local row
    float *best;             // [rows]; NULL: not wanted (q0 = 0 only)
    uint32_t rows;
    uint32_t n_q;            // vectors of this launch, 1 .. QP
    uint32_t q0;             // index of the launch's first vector within the call; != 0: merge with the stored pair
};

constexpr uint32_t ASSIGN_LDS_WORDS = 16384u;  // 64 KiB of x, whatever the tier
constexpr int assign_vectors_per_pass(int xcols) { return (int)ASSIGN_LDS_WORDS / xcols; }

// Vectors Q .. min(n_q, QP) - 1 of the launch against one packet: the recursion IS the compile-time unrolling (row_end_masks' idiom), so
// carry[Q] is a named scalar. A launch with fewer than QP vectors leaves at a wave-uniform branch.
template <int C, int XCOLS, int QM, int QP, int Q = 0>
__device__ __forceinline__ void assign_vectors(const Pkt<C, value_type_of(QM)> &cur, const uint32_t fl, const uint32_t n_q, const uint32_t xbase,
                                               float (&carry)[QP], float (&bst)[C], uint32_t (&lab)[C]) {
    if (Q != 0 && (uint32_t)Q >= n_q) return;
    // (copy Q's base is a constant that the 12-bit layout's address instruction wants in a scalar register: made where it is used --
    //  sixteen of them hoisted out of the packet loop were what the scalar file could not hold beside the scan's lane masks)
    uint32_t base = xbase + (uint32_t)Q * 4u * (uint32_t)XCOLS;
    asm volatile("" : "+s"(base));
    const Reduced<C> Rd = reduce_packet<C, QM>(cur, carry[Q], base, 0u);
    // (reduce_core hands the carry back out of v_readlane, a scalar register; sixteen of them beside the scan's lane masks are more
    //  than the scalar file holds -- 23 spilled when tried --, so a carry waits for its next packet in a vector register)
    asm("" : "+v"(carry[Q]));
    const RowSums<C> S = expand<C, false>(Rd, fl);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const bool better = Q == 0 || S.rs[j] > bst[j];
        bst[j] = better ? S.rs[j] : bst[j];
        lab[j] = better ? (uint32_t)Q : lab[j];
    }
    if constexpr (Q + 1 < QP) assign_vectors<C, XCOLS, QM, QP, Q + 1>(cur, fl, n_q, xbase, carry, bst, lab);
}

template <int C, int XCOLS, int QM>
__global__ void __launch_bounds__(512, 4) assign_kernel(const StreamParams P, const AssignParams R) {
    static_assert((QM == QM_F32 || QM == QM_F32C12) && (C == 4 || C == 8), "assign_kernel: fp32 packet streams of 4 or 8 entries per lane");
    static_assert(XCOLS % 512 == 0 && ASSIGN_LDS_WORDS % XCOLS == 0, "x is staged by 512 threads, whole copies");
    constexpr int VT = value_type_of(QM);
    constexpr int QP = assign_vectors_per_pass(XCOLS);
    constexpr bool BUF = C == 4;           // buffer loads (load_packet_buf) where they exist
    constexpr int NBUF = C == 8 ? 2 : 3;   // range_kernel's packet buffers
    constexpr uint32_t XPT = (uint32_t)XCOLS / 512u;  // words of one x per thread
    // (the kernel's ONLY __shared__ block: it starts at LDS address 0, so copy q starts on a 4 KiB boundary)
    __shared__ float xl[ASSIGN_LDS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bid = blockIdx.x, n_wg = gridDim.x;
    const uint32_t total_waves = (blockDim.x >> 6) * n_wg;
    const uint32_t part0 = wave * n_wg + bid;
    const uint32_t xbase = lds_addr_of(xl);
    const uint32_t n_q = R.n_q < (uint32_t)QP ? R.n_q : (uint32_t)QP;

    // the launch's vectors (clamped addresses, masked values)
    for (uint32_t q = 0; q < n_q; ++q) {
        const float *x = R.xs + (size_t)q * P.cols;
#pragma unroll
        for (uint32_t t = 0; t < XPT; ++t) {
            const uint32_t i = tid + 512u * t;
            const float xw = x[i < P.cols ? i : 0u];
            xl[q * (uint32_t)XCOLS + i] = i < P.cols ? xw : 0.0f;
        }
    }
    __syncthreads();

    Pkt<C, VT> buf[NBUF];
    LaneOffsets lo{0u, 0u};
    if constexpr (BUF) lo = lane_offsets<C, VT>(lane);
    const uint8_t *pk = R.packets;
    __amdgpu_buffer_rsrc_t rsrc = stream_resource(pk, 0u);
    uint32_t req_off = 0u;

    for (uint32_t part = part0; part < P.n_parts; part += total_waves) {
        uint32_t f0 = 0u, n = 0u;
        TKSPMV_PARTITION_RANGE(P, part, f0, n);
        // (wave-uniform by construction; said so, or every packet offset becomes a vector value: row_stats_kernel)
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
        float carry[QP];  // one per vector (a partition starts on a row boundary); indexed by unrolled constants only
#pragma unroll
        for (int q = 0; q < QP; ++q) carry[q] = 0.0f;
        // NBUF - 1 packets in flight behind the one being reduced; the buffers rotate by NAME (the loop is unrolled by NBUF).
        for (uint32_t i0 = 0; i0 < n; i0 += NBUF) {
#pragma unroll
            for (int u = 0; u < NBUF; ++u) {
                const uint32_t i = i0 + (uint32_t)u;
                if (i >= n) break;
                const Pkt<C, VT> &cur = buf[u];
                // Unconditional (offset clamped to the last packet): a fixed number of younger loads, as in row_stats_kernel.
                if constexpr (BUF) load_packet_buf<C, VT>(rsrc, req_off, lo, buf[(u + NBUF - 1) % NBUF]);
                else load_packet<C, VT>(pk + req_off, lane, buf[(u + NBUF - 1) % NBUF]);
                if (i + (uint32_t)NBUF < n) req_off += P.packet_bytes;
                const uint32_t rb = scalar_load(P.pkt_row + f0 + i);  // first row of the packet (scalar cache: retires through lgkmcnt)

                const uint32_t fl = packet_flags<C, QM>(cur);
                float bst[C];
                uint32_t lab[C];
                assign_vectors<C, XCOLS, QM, QP>(cur, fl, n_q, xbase, carry, bst, lab);
                uint32_t r = rb;  // + the row ends in lower lanes (ends_below, on the flag word)
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const uint64_t b = __ballot(((fl >> j) & 1u) != 0u);
                    r += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                }
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    // (r < rows always holds for a stream the packers wrote; the comparison keeps a damaged table from writing outside the outputs)
                    if (((fl >> j) & 0x101u) == 1u && r < R.rows) {
                        if (R.q0 == 0u) {
                            R.labels[r] = lab[j];
                            if (R.best) R.best[r] = bst[j];
                        } else if (bst[j] > R.best[r]) {
                            R.labels[r] = lab[j] + R.q0;
                            R.best[r] = bst[j];
                        }
                    }
                    r += (fl >> j) & 1u;
                }
            }
        }
    }
}

}  // namespace tkspmv
