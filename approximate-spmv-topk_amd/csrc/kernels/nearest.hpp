// kernels/nearest.hpp -- nearest_fill_kernel and nearest_kernel: for every stored row the n best-scoring of a set of vectors, in
// order, under an optional allow-mask of rows (tkspmv_enqueue_nearest): labels[rows][n] and scores[rows][n].
// Part of engine.hip (one translation unit: included there behind assign.hpp; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"
#include "assign.hpp"

namespace tkspmv {

// assign_kernel's loop (kernels/assign.hpp: one pass over stream copy 0, up to QP = 16384 / XCOLS vectors staged side by side in ONE
// static block of 64 KiB at LDS address 0, reduce_packet with one carry per vector, then expand -- the calls, the order and hence the
// bits of every other streaming path --, the vectors unrolled at compile time) keeping, per row-end slot, not one pair but a list of N
// pairs (score, label) sorted by score descending: vector Q goes in behind every entry whose score is >= its own, so equal scores
// (-0.0 and +0.0 among them) stay in the order of their indices. The lists are indexed by unrolled constants only -- named registers,
// never a run-time-indexed array, which would live in scratch. While the list is not full (Q < N) its length is the compile-time Q:
// the empty entries take no part in a comparison, so a score of -inf is placed like any other.
// N is 1, 2 or 4; a call with n entries per row runs the next N and stores the first n (N = 1 is assign_kernel's running pair). Entries no vector of the launch filled hold
// (NEAREST_NONE, -inf), the contract's padding.
// Stores: a row's list is contiguous, labels[r * n + j]. The first launch of a call (q0 = 0) stores its list as it is; a later one, at
// vector offset q0, loads the row's stored list, inserts its own entries behind it by the same rule -- stored entries have the smaller
// indices, so they come first on a tie; an empty entry (label NEAREST_NONE) yields to every score --, and stores the first n, its own
// labels offset by q0. One lane of one wave of one launch touches a row, and the launches of a call follow each other in stream order,
// so the read-modify-write needs no atomics.
// The allow-mask is honoured at the store: the storing lane loads the word of its row (bit r & 31 of word r >> 5) and a row outside
// the mask is never written. (Not range_kernel's scalar route, mask_pair + mask_rows: its two prefetched words per packet and its
// uniform loop over the further words of a packet that ends more than 33 .. 64 rows live in scalar registers, and this kernel's
// scalar file is full at N = 4; a lane's load needs none, only the storing lanes issue one, and they hold consecutive rows, so the
// words of a packet come from one or two cache lines.)
// Rows the kernel never stores to -- placeholders of empty rows, rows without packets, rows outside the mask -- hold what
// nearest_fill_kernel wrote in front of the first launch, on the same stream.
// Reads stream copy 0, pkt_row and the mask; writes labels and scores only. No engine state.
struct NearestParams {
    const uint8_t *packets;  // stream copy 0
    const float *xs;         // vector i of the launch: xs + i * cols
    const uint32_t *mask;    // allow-mask, bit r & 31 of word r >> 5; NULL: every row
    uint32_t *labels;        // [rows][n], indexed by local row
    float *scores;           // [rows][n]
    uint32_t rows;
    uint32_t n;              // entries per row, 1 .. N
    uint32_t n_q;            // vectors of this launch, 1 .. QP
    uint32_t q0;             // index of the launch's first vector within the call; != 0: merge with the stored list
};

constexpr uint32_t NEAREST_NONE = 0xFFFFFFFFu;  // TKSPMV_NEAREST_NONE
constexpr float NEAREST_NO_SCORE = -__builtin_inff();

// The default list of every row, in front of a call's first streaming launch: an eligible row (in the mask, or no mask) gets the list
// of a row without entries -- +0.0f against every vector, so labels 0, 1, .. up to count, then padding --, a row outside the mask
// padding throughout. One thread per output word pair, grid-stride.
__global__ void __launch_bounds__(256) nearest_fill_kernel(const uint32_t *mask, uint32_t *labels, float *scores, const uint32_t rows, const uint32_t n,
                                                           const uint32_t count) {
    const uint64_t total = (uint64_t)rows * n;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t r = (uint32_t)(i / n), j = (uint32_t)(i - (uint64_t)r * n);
        const bool eligible = !mask || ((mask[r >> 5] >> (r & 31u)) & 1u) != 0u;
        const bool zero = eligible && j < count;
        labels[i] = zero ? j : NEAREST_NONE;
        scores[i] = zero ? 0.0f : NEAREST_NO_SCORE;
    }
}

// (s, q) into a list of LEN entries sorted by score descending (LEN = N: full, its last entry drops out; LEN < N: entry LEN is
// empty and takes the new pair first), behind every entry whose score is >= s: the new pair climbs from the bottom while the entry
// above it scores less. Each comparison is used at once -- one lane mask alive at a time, the scalar file has no room for N of them
// per slot beside the scan's.
template <int N, int LEN>
__device__ __forceinline__ void nearest_insert(float (&sc)[N], uint32_t (&lb)[N], const float s, const uint32_t q) {
    if constexpr (LEN < N) {
        sc[LEN] = s;
        lb[LEN] = q;
    }
#pragma unroll
    for (int i = LEN - 1; i >= 0; --i) {
        const bool up = s > sc[i];  // (false once, false from there on: the list is sorted)
        if (i + 1 < N) {
            sc[i + 1] = up ? sc[i] : sc[i + 1];
            lb[i + 1] = up ? lb[i] : lb[i + 1];
        }
        sc[i] = up ? s : sc[i];
        lb[i] = up ? q : lb[i];
    }
}

// The merge launches' insertion: entry (s, q) of the launch's own list into the stored list, whose empty entries (label
// NEAREST_NONE) yield to every score; an empty entry of the own list (q = NEAREST_NONE) is not inserted. q0: the launch's offset.
template <int N>
__device__ __forceinline__ void nearest_merge_one(float (&ts)[N], uint32_t (&tl)[N], const float s, const uint32_t q, const uint32_t q0) {
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        const bool up = q != NEAREST_NONE && (tl[i] == NEAREST_NONE || s > ts[i]);
        if (i + 1 < N) {
            ts[i + 1] = up ? ts[i] : ts[i + 1];
            tl[i + 1] = up ? tl[i] : tl[i + 1];
        }
        ts[i] = up ? s : ts[i];
        tl[i] = up ? q + q0 : tl[i];
    }
}

// Vectors Q .. min(n_q, QP) - 1 of the launch against one packet: assign_vectors' recursion with a list per slot.
template <int C, int XCOLS, int QM, int QP, int N, int Q = 0>
__device__ __forceinline__ void nearest_vectors(const Pkt<C, value_type_of(QM)> &cur, const uint32_t fl, const uint32_t n_q, const uint32_t xbase,
                                                float (&carry)[QP], float (&sc)[C][N], uint32_t (&lb)[C][N]) {
    // (n_q through an empty asm: compared here, on the scalar unit, each time -- or the fifteen comparisons are made once, in front of
    //  the packet loop, and kept as fifteen lane masks in thirty scalar registers that the loop has not got)
    if constexpr (Q != 0) {
        uint32_t nq = n_q;
        asm volatile("" : "+s"(nq));
        if ((uint32_t)Q >= nq) return;
    }
    // (copy Q's base made where it is used, the carry kept in a vector register between packets: assign_vectors says why)
    uint32_t base = xbase + (uint32_t)Q * 4u * (uint32_t)XCOLS;
    asm volatile("" : "+s"(base));
    const Reduced<C> Rd = reduce_packet<C, QM>(cur, carry[Q], base, 0u);
    asm("" : "+v"(carry[Q]));
    const RowSums<C> S = expand<C, false>(Rd, fl);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        if constexpr (Q == 0) {
            sc[j][0] = S.rs[j];
            lb[j][0] = 0u;
#pragma unroll
            for (int i = 1; i < N; ++i) {
                sc[j][i] = NEAREST_NO_SCORE;
                lb[j][i] = NEAREST_NONE;
            }
        } else {
            nearest_insert<N, (Q < N ? Q : N)>(sc[j], lb[j], S.rs[j], (uint32_t)Q);
        }
    }
    if constexpr (Q + 1 < QP) nearest_vectors<C, XCOLS, QM, QP, N, Q + 1>(cur, fl, n_q, xbase, carry, sc, lb);
}

// Workgroups per CU the kernel is built for: two (at most 128 registers) except where the lists of 8 slots x 4 entries do not fit
// beside the 8-entries-per-lane scan -- that instantiation takes one workgroup's registers rather than spill.
constexpr int nearest_waves_per_eu(int c, int n) { return c == 8 && n == 4 ? 2 : 4; }

template <int C, int XCOLS, int QM, int N>
__global__ void __launch_bounds__(512, nearest_waves_per_eu(C, N)) nearest_kernel(const StreamParams P, const NearestParams R) {
    static_assert((QM == QM_F32 || QM == QM_F32C12) && (C == 4 || C == 8), "nearest_kernel: fp32 packet streams of 4 or 8 entries per lane");
    static_assert(XCOLS % 512 == 0 && ASSIGN_LDS_WORDS % XCOLS == 0, "x is staged by 512 threads, whole copies");
    static_assert(N == 1 || N == 2 || N == 4, "lists of 1, 2 or 4 entries");
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
    const uint32_t n_out = R.n < (uint32_t)N ? R.n : (uint32_t)N;

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
                float sc[C][N];
                uint32_t lb[C][N];
                nearest_vectors<C, XCOLS, QM, QP, N>(cur, fl, n_q, xbase, carry, sc, lb);
                uint32_t r = rb;  // + the row ends in lower lanes (ends_below, on the flag word)
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const uint64_t b = __ballot(((fl >> j) & 1u) != 0u);
                    r += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                }
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    // (r < rows always holds for a stream the packers wrote; the comparison keeps a damaged table from writing outside the
                    //  outputs -- and from reading outside the mask)
                    if (((fl >> j) & 0x101u) == 1u && r < R.rows && (!R.mask || ((R.mask[r >> 5] >> (r & 31u)) & 1u) != 0u)) {
                        uint32_t *const ol = R.labels + (size_t)r * R.n;
                        float *const os = R.scores + (size_t)r * R.n;
                        if (R.q0 == 0u) {
#pragma unroll
                            for (int i = 0; i < N; ++i) {
                                if ((uint32_t)i < n_out) {
                                    ol[i] = lb[j][i];
                                    os[i] = sc[j][i];
                                }
                            }
                        } else {
                            // the stored list (entries behind n: empty), then this launch's entries behind their equals
                            float ts[N];
                            uint32_t tl[N];
#pragma unroll
                            for (int i = 0; i < N; ++i) {
                                const bool have = (uint32_t)i < n_out;
                                tl[i] = have ? ol[i] : NEAREST_NONE;
                                ts[i] = have ? os[i] : NEAREST_NO_SCORE;
                            }
#pragma unroll
                            for (int k = 0; k < N; ++k) nearest_merge_one<N>(ts, tl, sc[j][k], lb[j][k], R.q0);
#pragma unroll
                            for (int i = 0; i < N; ++i) {
                                if ((uint32_t)i < n_out) {
                                    ol[i] = tl[i];
                                    os[i] = ts[i];
                                }
                            }
                        }
                    }
                    r += (fl >> j) & 1u;
                }
            }
        }
    }
}

}  // namespace tkspmv
