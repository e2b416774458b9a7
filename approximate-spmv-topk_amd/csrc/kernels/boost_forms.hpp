// kernels/boost_forms.hpp -- Boosted range and facet queries: the per-row transform of a query's scores fused with the threshold and
// the sink (boosted_hits_kernel, boosted_bins_kernel). Part of engine.hip (one translation unit: included there only; device code only).
#pragma once
#include "boost_cut.hpp"

namespace tkspmv {
namespace boost_forms {

using boost_kernels::boosted_score;
using boost_kernels::BOOST_LANE_ROWS;
using boost_kernels::BOOST_THREADS;
using boost_kernels::BOOST_TILE;

// ------------------------------------------------------------------------------------------------------------
// A boosted threshold cannot be tested per packet: range_kernel's and facet_kernel's trigger bounds the RAW sums of a packet's rows,
// and weight and bias differ by row. So these forms take the search-after route: the SpMV-only kernel writes every row's score into
// the engine's array, and ONE pass over that array transforms, compares and delivers. With s the score in the array,
//     s' = boosted_score(s, weight[r], bias[r])      (boost_cut.hpp: two separately rounded operations; -inf stays, non-finite -> -inf)
// and row r matches when s' > -inf and s' >= threshold, compared as floats (a threshold of -inf: every row with a finite s'; NaN:
// none). The array is read only: nothing is stored back, no selection follows.
// ------------------------------------------------------------------------------------------------------------
struct ScanParams {
    const float *y;          // [rows] the scores of the query in flight, -inf where a row has no entry or the mask excludes it
    const float *weight;     // [rows] by LOCAL row, or NULL: no multiply
    const float *bias;       // [rows] by LOCAL row, or NULL: no add
    const float *threshold;  // the query's threshold, one float in device memory
    uint32_t wide;           // both arrays (where given) start at a multiple of 16 bytes: a lane's four rows are one load each
    uint32_t rows, first_row;
};
struct HitsParams {
    ScanParams S;
    uint32_t *idx;     // [capacity] global row ids of the matches, or NULL with capacity = 0
    float *val;        // [capacity] their boosted scores
    uint32_t capacity;
    uint32_t *count;   // the query's counter: all matches, also those beyond capacity; zeroed in front
};
struct BinsParams {
    ScanParams S;
    const uint32_t *labels;    // [rows] label of each local row; >= n_bins: the row belongs to no bin
    uint32_t wide_labels;      // labels start at a multiple of 16 bytes
    uint32_t n_bins;
    uint32_t in_lds;           // != 0: the workgroup-private histogram (the launch gives n_bins * 12 bytes of LDS)
    uint32_t *counts;          // [n_bins] matches per bin; zeroed in front
    unsigned long long *best;  // [n_bins] maximum of (order key << 32 | global row) per bin, or NULL; zeroed in front
    uint32_t *total;           // all matches, or NULL; zeroed in front
};
// Bins the workgroup-private histogram of boosted_bins_kernel holds at most, 12 bytes each: 48 KiB, three workgroups per CU at the
// limit. The LDS is sized per launch (n_bins * 12 bytes), so a call of few bins keeps all eight workgroups on the CU.
constexpr uint32_t BINS_LDS_CAP = 4096u;

// boost_cut_kernel's geometry and loads: lane <-> four consecutive rows of a tile of 256, 16-byte loads of the scores (the engine's own
// allocation) and, where the host found the caller's arrays aligned, of weight and bias; the lane that holds the matrix' last rows
// loads one by one, and so does every lane for arrays that are not aligned. A slot beyond the last row holds -inf: it matches nothing.
__device__ __forceinline__ void boosted_tile(const ScanParams &S, uint64_t r0, bool full, float (&v)[BOOST_LANE_ROWS]) {
    const bool has_w = S.weight != nullptr, has_b = S.bias != nullptr;
    float sc[BOOST_LANE_ROWS], w[BOOST_LANE_ROWS], b[BOOST_LANE_ROWS];
    if (full) {
        const float4 s4 = *reinterpret_cast<const float4 *>(S.y + r0);
        sc[0] = s4.x, sc[1] = s4.y, sc[2] = s4.z, sc[3] = s4.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) sc[j] = r0 + j < (uint64_t)S.rows ? S.y[r0 + j] : -__builtin_huge_valf();
    }
    if (full && S.wide != 0u) {
        const float4 w4 = has_w ? *reinterpret_cast<const float4 *>(S.weight + r0) : float4{1.0f, 1.0f, 1.0f, 1.0f};
        const float4 b4 = has_b ? *reinterpret_cast<const float4 *>(S.bias + r0) : float4{0.0f, 0.0f, 0.0f, 0.0f};
        w[0] = w4.x, w[1] = w4.y, w[2] = w4.z, w[3] = w4.w;
        b[0] = b4.x, b[1] = b4.y, b[2] = b4.z, b[3] = b4.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) {
            const bool in = r0 + j < (uint64_t)S.rows;
            w[j] = has_w && in ? S.weight[r0 + j] : 1.0f;
            b[j] = has_b && in ? S.bias[r0 + j] : 0.0f;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) v[j] = boosted_score(sc[j], w[j], b[j], has_w, has_b);
}

__device__ __forceinline__ bool boosted_match(float v, float tau) { return v > -__builtin_huge_valf() && v >= tau; }  // (NaN compares false)

// Range sink: per tile four ballots, one relaxed agent-scope add per wave that has matches -- it reserves the wave's positions in the
// query's counter --, then the stores of the pairs whose position is below capacity. The counter goes on counting beyond capacity.
__global__ void __launch_bounds__(BOOST_THREADS) boosted_hits_kernel(const HitsParams H) {
    const ScanParams &S = H.S;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * BOOST_THREADS + threadIdx.x) >> 6, n_waves = gridDim.x * (BOOST_THREADS / 64u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)S.rows + BOOST_TILE - 1u) / BOOST_TILE);
    const float tau = *S.threshold;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {  // wave-uniform
        const uint64_t r0 = (uint64_t)t * BOOST_TILE + lane * BOOST_LANE_ROWS;  // (64 bits: the last tile may reach past 2^32)
        float v[BOOST_LANE_ROWS];
        boosted_tile(S, r0, r0 + BOOST_LANE_ROWS <= (uint64_t)S.rows, v);
        bool hit[BOOST_LANE_ROWS];
        uint32_t before[BOOST_LANE_ROWS], n = 0u;  // n: the tile's matches (wave-uniform)
#pragma unroll
        for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) {
            hit[j] = boosted_match(v[j], tau);
            const unsigned long long bal = __ballot(hit[j]);
            before[j] = n + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            n += (uint32_t)__popcll(bal);
        }
        if (n == 0u) continue;  // wave-uniform
        uint32_t base = 0u;
        if (lane == 0u) base = __hip_atomic_fetch_add(H.count, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= H.capacity) continue;  // (nothing of this tile is written; capacity = 0: never anything)
#pragma unroll
        for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) {
            const uint32_t pos = base + before[j];
            if (hit[j] && pos >= base && pos < H.capacity) {  // (pos >= base: a counter past 2^32 wraps, and writes nothing)
                H.idx[pos] = S.first_row + (uint32_t)(r0 + j);
                H.val[pos] = v[j];
            }
        }
    }
}

// Facet sink: a 16-byte load of four labels beside the scores, and a deposit per match into the bin of its label -- in the
// workgroup-private histogram (count and 64-bit key per bin, LDS atomics; cleared at entry, swept to counts / best with one global
// atomic per non-zero bin once the workgroup's tiles are done) or, for more bins than fit, with global atomics directly. The regime is
// a launch parameter (wave-uniform). A label beyond the bins counts in the total only; the total costs one atomic per wave.
// facet_close_kernel turns the keys into the caller's records behind this kernel.
__global__ void __launch_bounds__(BOOST_THREADS) boosted_bins_kernel(const BinsParams B) {
    extern __shared__ unsigned long long bins_lds[];  // [n_bins] keys, then [n_bins] counts (in_lds only)
    const ScanParams &S = B.S;
    const bool in_lds = B.in_lds != 0u, want_best = B.best != nullptr;
    unsigned long long *const hbest = bins_lds;
    uint32_t *const hcount = reinterpret_cast<uint32_t *>(bins_lds + B.n_bins);
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < B.n_bins; b += BOOST_THREADS) {
            hbest[b] = 0ull;
            hcount[b] = 0u;
        }
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * BOOST_THREADS + threadIdx.x) >> 6, n_waves = gridDim.x * (BOOST_THREADS / 64u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)S.rows + BOOST_TILE - 1u) / BOOST_TILE);
    const float tau = *S.threshold;
    uint32_t seen = 0u;  // matches this wave has seen (wave-uniform)
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {  // wave-uniform
        const uint64_t r0 = (uint64_t)t * BOOST_TILE + lane * BOOST_LANE_ROWS;
        const bool full = r0 + BOOST_LANE_ROWS <= (uint64_t)S.rows;
        float v[BOOST_LANE_ROWS];
        boosted_tile(S, r0, full, v);
        uint32_t lab[BOOST_LANE_ROWS];
        if (full && B.wide_labels != 0u) {
            const uint4 l4 = *reinterpret_cast<const uint4 *>(B.labels + r0);
            lab[0] = l4.x, lab[1] = l4.y, lab[2] = l4.z, lab[3] = l4.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) lab[j] = r0 + j < (uint64_t)S.rows ? B.labels[r0 + j] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t j = 0; j < BOOST_LANE_ROWS; ++j) {
            const bool hit = boosted_match(v[j], tau);
            seen += (uint32_t)__popcll(__ballot(hit));
            if (hit && lab[j] < B.n_bins) {
                const unsigned long long key = ((unsigned long long)order_key(v[j]) << 32) | (unsigned long long)(S.first_row + (uint32_t)(r0 + j));
                if (in_lds) {
                    (void)__hip_atomic_fetch_add(&hcount[lab[j]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (want_best) (void)__hip_atomic_fetch_max(&hbest[lab[j]], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    (void)__hip_atomic_fetch_add(B.counts + lab[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (want_best) (void)__hip_atomic_fetch_max(B.best + lab[j], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    if (B.total != nullptr && lane == 0u && seen != 0u) (void)__hip_atomic_fetch_add(B.total, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (in_lds) {
        __syncthreads();  // (every wave's deposits are in)
        for (uint32_t b = threadIdx.x; b < B.n_bins; b += BOOST_THREADS) {
            const uint32_t c = hcount[b];
            if (c != 0u) {
                (void)__hip_atomic_fetch_add(B.counts + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (want_best) (void)__hip_atomic_fetch_max(B.best + b, hbest[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

}  // namespace boost_forms
}  // namespace tkspmv
