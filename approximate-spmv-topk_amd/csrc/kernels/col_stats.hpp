// kernels/col_stats.hpp -- col_stats_kernel: one statistic of every COLUMN over the rows of a set (tkspmv_enqueue_col_stats): the number
// of stored entries, or the largest / smallest stored value.
// Part of engine.hip (one translation unit: included there behind the other kernel headers; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"
#include "match_kernel.hpp"  // col_offset

namespace tkspmv {

// match_kernel's launch (512 threads over the engine's grid and wave partitions, packets prefetched through buffer loads with counted
// waits, a set per query slot, no workgroup ever waits for another) with facet_kernel's sink: a workgroup-private array of XCOLS words in
// LDS, one LDS atomic per counted entry at the entry's column, swept to global memory with agent-scope atomics behind the workgroup's
// last partition of a set.
//   EXT = false (TKSPMV_COL_NNZ): add 1. Only the column plane of a packet travels (the flags ride in it).
//   EXT = true  (TKSPMV_COL_MAX / _MIN): max of order_key(v ^ negate); negate = the sign bit for MIN -- the smallest value is the largest
//     of the negated ones --, undone by col_stats_close_kernel, which turns keys back into floats (key 0, which order_key gives no
//     finite or infinite float: -inf, +inf for MIN).
// Integer add and max are associative and commutative: the result does not depend on the geometry or on the order of the atomics.
// An entry is COUNTED when it is none of
//   - the placeholder of an empty row (SKIP, bit 8 + j of the flag word);
//   - padding: a slot behind its partition's last row end (column word 0, value +0.0, no flags -- it looks like an entry of column 0).
//     Before the loop the wave reads the flags of the partition's last packet, walks back while a packet holds no row end, and keeps
//     the wave-uniform pair (last packet, last slot); packets behind it are not visited, slots behind it in it are not counted. (Not
//     through the mask: the row index of padding lies beyond the partition's rows.)
//   - FILT: an entry whose row the set's allow-mask excludes (mask_entries below).
// Reads the stream copies and, with FILT, pkt_row and the masks; writes out only. No engine state.
struct ColStatsParams {
    const uint8_t *replicas[16];  // the copies of the packet stream (cache-defeat mode); [0] alone otherwise
    uint32_t n_replicas;
    uint32_t q0;                  // number of this launch's first set within the call (picks the stream copies)
    uint32_t n_q;
    const uint32_t *mask;         // FILT: set i's allow-mask at mask + i * mask_stride words
    uint32_t mask_stride, mask_words;
    uint32_t *out;                // set i's result at out + i * out_stride words (cols of them, zeroed in front of the launch)
    uint64_t out_stride;
    uint32_t negate;              // EXT: 0x80000000 for MIN, 0 for MAX
    uint32_t args_tag;            // COL_STATS_ARGS_TAG: the kernel finds it where it expects R in its argument segment, or traps
};
constexpr uint32_t COL_STATS_ARGS_TAG = 0xC0157A75u;

// Which of the lane's C entries the mask allows (bit j: entry j). The row of entry j is rb + (row ends in lower lanes) + (row ends among
// the lane's entries 0 .. j-1): at most C consecutive rows r0, r0 + 1, ..., so two mask words picked in registers and one alignbit
// cover them -- the window of mask_rows, which works on row ENDS and stops one row short: an entry behind the packet's last row end
// belongs to row rb + n_ends, which continues in the next packet, and is counted under that row's bit. mw: mask_pair(F, rb); the words
// past rb's second are loaded here (clamped like mask_pair's: the loads never leave the mask), only for packets whose rows reach them.
template <int C>
__device__ __forceinline__ uint32_t mask_entries(uint32_t fl, uint32_t rb, uint2 mw, const FilterParams &F) {
    const uint32_t ends = (uint32_t)__popc(fl & ((1u << C) - 1u));
    uint32_t below = 0u, n_ends = 0u;
#pragma unroll
    for (int b = 0; (1 << b) <= C; ++b) {  // sums over the lanes of numbers of at most C, bit by bit (match_kernel)
        const uint64_t eb = __ballot(((ends >> b) & 1u) != 0u);
        below += __builtin_amdgcn_mbcnt_hi((uint32_t)(eb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)eb, 0u)) << b;
        n_ends += (uint32_t)__popcll(eb) << b;
    }
    const uint32_t r0 = rb + below;  // the row of the lane's entry 0
    const uint32_t wb = rb >> 5;
    const uint32_t lw = (r0 >> 5) - wb;  // the lane's first word, relative to wb
    uint32_t lo = lw == 0u ? mw.x : (lw == 1u ? mw.y : 0u);
    uint32_t hi = lw == 0u ? mw.y : 0u;
    const uint32_t we = (rb + n_ends) >> 5;  // last word the packet's rows reach, the continuing row included (uniform)
    for (uint32_t w = wb + 2u; w <= we; ++w) {  // (a lane whose window starts in word we reads no bit of word we + 1: its rows end at rb + n_ends)
        const uint32_t s = scalar_load(F.mask + (w < F.words - 1u ? w : F.words - 1u));
        lo = (lw == w - wb) ? s : lo;
        hi = (lw + 1u == w - wb) ? s : hi;
    }
    uint32_t bits = __builtin_amdgcn_alignbit(hi, lo, r0 & 31u);  // bit t: row r0 + t
    uint32_t allow = 0u;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        allow |= (bits & 1u) << j;
        bits >>= (fl >> j) & 1u;
    }
    return allow;
}

// A lane's share of a packet through buffer loads, for 4 and for 8 entries per lane: the column plane (load_cols_buf's requests) and,
// with VALUES, one dwordx4 per plane of 4 values. Loads beyond the resource's length return 0 (never requested: the kernel clamps to
// the partition's last packet).
template <int C, int VT, bool VALUES>
__device__ __forceinline__ void load_stat_packet(__amdgpu_buffer_rsrc_t rsrc, uint32_t packet_off, uint32_t lane, uint32_t coff, Pkt<C, VT> &o) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
        if constexpr (VALUES) {
            const u32x4 f = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16u + (uint32_t)q * 1024u, packet_off, 2);  // (aux 2: non-temporal)
            o.v[4 * q + 0] = __uint_as_float(f.x);
            o.v[4 * q + 1] = __uint_as_float(f.y);
            o.v[4 * q + 2] = __uint_as_float(f.z);
            o.v[4 * q + 3] = __uint_as_float(f.w);
        }
        const u32x2 c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, coff + (uint32_t)q * 512u, packet_off, 2);
        o.cw[2 * q + 0] = c.x;
        o.cw[2 * q + 1] = c.y;
    }
}

// LDS byte offset of the word of entry j's column inside the array (always inside it: the field is cut to the tier's width).
template <int C, int XCOLS, int QM>
__device__ __forceinline__ uint32_t column_offset(const Pkt<C, value_type_of(QM)> &cur, int j) {
    constexpr uint32_t FIELD = ((uint32_t)XCOLS - 1u) << 2;
    if constexpr (QM == QM_F32C12) {  // A = col0 << 2 | col1 << 12 | col2 << 22 | flags, B = col3 << 2 | flags (packet_math.hpp)
        uint32_t A, B;
        split_ab(cur.cw[0], cur.cw[1], A, B);
        return (j == 0 ? A : j == 1 ? A >> 10 : j == 2 ? A >> 20 : B) & (FIELD & 0xFFCu);
    } else {
        return (cur.cw[j >> 1] >> (16 * (j & 1))) & FIELD;
    }
}

typedef __attribute__((address_space(3))) uint32_t lds_wu32;

template <int C, int XCOLS, bool C12, bool EXT, bool FILT>
__global__ void __launch_bounds__(512, 4) col_stats_kernel(const StreamParams P, const ColStatsParams R) {
    static_assert((C == 4 || C == 8) && (!C12 || C == 4), "col_stats_kernel: fp32 packet streams of 4 or 8 entries per lane");
    static_assert(XCOLS % 512 == 0 && XCOLS * 4 <= 80 * 1024, "the array is swept by 512 threads; two workgroups per CU");
    constexpr int QM = C12 ? QM_F32C12 : QM_F32;
    constexpr int VT = value_type_of(QM);
    constexpr int NBUF = EXT ? (C == 8 ? 2 : 3) : 4;  // range_kernel's packet buffers for whole packets, match_kernel's for column planes
    constexpr uint32_t PE = 64u * (uint32_t)C;
    __shared__ uint32_t hist[XCOLS];  // the kernel's only __shared__ block: LDS offset 0
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bid = blockIdx.x, n_wg = gridDim.x;
    const uint32_t total_waves = (blockDim.x >> 6) * n_wg;
    const uint32_t part0 = wave * n_wg + bid;
    const uint32_t hbase = lds_addr_of(hist);
    const uint32_t coff = col_offset<C, VT>(lane);

    for (uint32_t c = tid; c < (uint32_t)XCOLS; c += 512u) hist[c] = 0u;
    __syncthreads();

    // R as it lies in the kernel's argument segment, behind P (facet_kernel has the rule relied on and its guards): the table of stream
    // copies is indexed at run time, which on the by-value copy would put the whole block into scratch memory.
    typedef const char __attribute__((address_space(4))) *ArgBytes;
    typedef const ColStatsParams __attribute__((address_space(4))) *ColStatsArgs;
    static_assert(sizeof(StreamParams) % alignof(ColStatsParams) == 0, "R follows P without padding");
    const ColStatsArgs A = (ColStatsArgs)((ArgBytes)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(StreamParams));
    if (A->args_tag != COL_STATS_ARGS_TAG || A->n_q != R.n_q || A->mask_words != R.mask_words) __builtin_trap();

    Pkt<C, VT> buf[NBUF];
    for (uint32_t q = 0; q < R.n_q; ++q) {
        const uint8_t *const packets = A->replicas[(R.q0 + q) % R.n_replicas];
        const FilterParams F{FILT ? R.mask + (size_t)q * R.mask_stride : nullptr, R.mask_words};
        for (uint32_t part = part0; part < P.n_parts; part += total_waves) {
            uint32_t f0 = 0u, n_all = 0u;
            TKSPMV_PARTITION_RANGE(P, part, f0, n_all);
            // (wave-uniform by construction; said so, or every packet offset becomes a vector value: row_stats_kernel)
            f0 = __builtin_amdgcn_readfirstlane(f0);
            n_all = __builtin_amdgcn_readfirstlane(n_all);
            // The first NBUF - 1 packets (clamped to the partition's last packet; a partition without packets has a resource of 0
            // bytes, whose loads return 0 and touch nothing).
            const __amdgpu_buffer_rsrc_t rsrc = stream_resource(packets + (size_t)f0 * P.packet_bytes, n_all * P.packet_bytes);
#pragma unroll
            for (int u = 0; u < NBUF - 1; ++u) {
                const uint32_t iu = ((uint32_t)u < n_all) ? (uint32_t)u : (n_all > 0u ? n_all - 1u : 0u);
                load_stat_packet<C, VT, EXT>(rsrc, iu * P.packet_bytes, lane, coff, buf[u]);
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
            // NBUF - 1 packets in flight behind the one being counted; the buffers rotate by NAME (the loop is unrolled by NBUF).
            for (uint32_t i0 = 0; i0 < n; i0 += NBUF) {
#pragma unroll
                for (int u = 0; u < NBUF; ++u) {
                    const uint32_t i = i0 + (uint32_t)u;
                    if (i >= n) break;
                    const Pkt<C, VT> &cur = buf[u];
                    // Unconditional (offset clamped to the last packet): a fixed number of younger loads lets the compiler wait with a
                    // counted vmcnt instead of vmcnt(0).
                    load_stat_packet<C, VT, EXT>(rsrc, req_off, lane, coff, buf[(u + NBUF - 1) % NBUF]);
                    if (i + (uint32_t)NBUF < n_all) req_off += P.packet_bytes;

                    const uint32_t fl = packet_flags<C, QM>(cur);
                    // slots of the lane that lie in front of the padding: entry j iff lane * C + j <= last_slot in the last packet
                    const uint32_t lim = i + 1u == n ? last_slot : PE - 1u;
                    const uint32_t lc = lane * (uint32_t)C;
                    const uint32_t live = lim < lc ? 0u : (lim - lc >= (uint32_t)C - 1u ? (1u << C) - 1u : (2u << (lim - lc)) - 1u);
                    uint32_t counted = live & ~(fl >> 8);
                    if constexpr (FILT) {
                        const uint32_t rb = scalar_load(P.pkt_row + f0 + i);  // first row of the packet
                        counted &= mask_entries<C>(fl, rb, mask_pair(F, rb), F);
                    }
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        if ((counted >> j) & 1u) {
                            lds_wu32 *const w = reinterpret_cast<lds_wu32 *>((uintptr_t)(hbase + column_offset<C, XCOLS, QM>(cur, j)));
                            if constexpr (EXT) (void)__hip_atomic_fetch_max(w, order_key(__uint_as_float(__float_as_uint(cur.v[j]) ^ R.negate)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            else (void)__hip_atomic_fetch_add(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            }
        }
        // The workgroup's array of set q to global memory, non-zero words only, each cleared by the thread that swept it (facet_kernel's
        // flush); the second barrier keeps a wave that is through from depositing the next set's entries into words not swept yet.
        __syncthreads();
        uint32_t *const out_q = R.out + (size_t)q * R.out_stride;
        for (uint32_t c = tid; c < (uint32_t)XCOLS; c += 512u) {
            const uint32_t v = hist[c];
            if (v != 0u) {
                hist[c] = 0u;
                if (c < P.cols) {  // (always, for a stream the packers wrote: the comparison keeps a damaged one from writing outside out)
                    if constexpr (EXT) (void)__hip_atomic_fetch_max(out_q + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else (void)__hip_atomic_fetch_add(out_q + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (q + 1u < R.n_q) __syncthreads();
    }
}

// Closing launch over the sets' words of a MAX / MIN call: an order key becomes the float it stands for, key 0 (no counted entry)
// -inf; then the negation of MIN is undone (+inf for its empty columns). Set i at out + i * out_stride words, cols of them.
__global__ void __launch_bounds__(256) col_stats_close_kernel(uint32_t *out, uint64_t out_stride, uint32_t cols, uint32_t n_sets, uint32_t negate) {
    const unsigned long long n = (unsigned long long)cols * n_sets;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256u) {
        uint32_t *const w = out + (i / cols) * out_stride + (i % cols);
        const uint32_t k = *w;
        *w = (k != 0u ? __float_as_uint(key_to_float(k)) : 0xFF800000u) ^ negate;
    }
}

}  // namespace tkspmv
