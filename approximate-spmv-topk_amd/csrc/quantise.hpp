// quantise.hpp -- the fixed-point grid of the label sums (tkspmv_enqueue_label_sums): one function, compiled for the device
// (kernels/label_sums.hpp) and for the host (packed_host.cpp), so that both sides add the same integers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TKSPMV_HOST_DEVICE __host__ __device__
#else
#define TKSPMV_HOST_DEVICE
#endif

namespace tkspmv {

// The largest shift the call is defined for (s = x - E below): 24 significand bits shifted by 38 stay below 2^62.
constexpr int32_t QUANTISE_MAX_SHIFT = 38;

// The value with fp32 bit pattern `bits` as a multiple of 2^E, rounded to nearest with ties to even on the magnitude:
//   |v| = m * 2^x, m the 24-bit significand (a subnormal: no hidden bit, x = -149); s = x - E;
//   s >= 0: q = m << s;  s < 0: q = m >> -s, rounded (a shift of 64 or more gives 0);  the result takes the sign of v.
// Integer arithmetic on the bit pattern only: no floating-point instruction takes part, so denormal modes and contraction cannot make
// host and device differ, and quantise(-v) = -quantise(v). Defined for finite v with s <= QUANTISE_MAX_SHIFT. Inf, NaN and larger
// shifts give unspecified words; both shifts are clamped, so nothing is undefined behaviour.
TKSPMV_HOST_DEVICE inline int64_t quantise(uint32_t bits, int32_t E) {
    const uint32_t e = (bits >> 23) & 0xFFu;
    const uint64_t m = (uint64_t)(bits & 0x7FFFFFu) | (e != 0u ? 0x800000ull : 0ull);
    const int64_t s = (int64_t)(e != 0u ? (int32_t)e - 150 : -149) - (int64_t)E;
    uint64_t q;
    if (s >= 0) {
        q = m << (uint32_t)(s < 39 ? s : 39);  // (m < 2^24: no bit is lost)
    } else {
        const uint32_t t = (uint32_t)(-s < 63 ? -s : 63);  // (m < 2^24 < half of 2^63: a shift of 63 rounds to 0 like every longer one)
        const uint64_t rem = m & ((1ull << t) - 1ull), half = 1ull << (t - 1u);
        q = m >> t;
        q += (rem > half || (rem == half && (q & 1ull) != 0ull)) ? 1ull : 0ull;
    }
    return (bits >> 31) != 0u ? -(int64_t)q : (int64_t)q;
}

// The default exponent E of a matrix whose largest |v| has the bit pattern max_abs_bits and whose fullest column holds max_col_nnz
// counted entries: E = xmax + 1 + ceil_log2(max(1, max_col_nnz)) - 62, xmax the unbiased exponent of the largest |v| (-126 for a
// subnormal or zero). Every |v| < 2^(xmax + 1), so a column's sum stays below 2^62 quanta plus half a quantum per entry: no sum
// reaches 2^63. A matrix without entries: 0.
TKSPMV_HOST_DEVICE inline int32_t sums_exponent_of(uint32_t max_abs_bits, uint32_t max_col_nnz) {
    if (max_col_nnz == 0u) return 0;
    const uint32_t e = (max_abs_bits >> 23) & 0xFFu;
    const int32_t xmax = e != 0u ? (int32_t)e - 127 : -126;
    int32_t lg = 0;
    while ((1ull << lg) < (uint64_t)max_col_nnz) ++lg;
    return xmax + 1 + lg - 62;
}

// ... from the three column statistics of the matrix (TKSPMV_COL_NNZ, _MAX, _MIN as words, cols of each): what tkspmv_sums_exponent
// and tkspmv_packed_sums_exponent answer. |v| as bits: the magnitudes of finite floats order like their bit patterns. A column
// without a counted entry holds -inf / +inf and is left out.
inline int32_t sums_exponent_of_columns(const uint32_t *nnz, const uint32_t *hi, const uint32_t *lo, size_t cols) {
    uint32_t max_nnz = 0u, max_abs = 0u;
    for (size_t c = 0; c < cols; ++c) {
        if (nnz[c] == 0u) continue;
        max_nnz = std::max(max_nnz, nnz[c]);
        max_abs = std::max({max_abs, hi[c] & 0x7FFFFFFFu, lo[c] & 0x7FFFFFFFu});
    }
    return sums_exponent_of(max_abs, max_nnz);
}

}  // namespace tkspmv
