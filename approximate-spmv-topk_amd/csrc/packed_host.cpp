// packed_host.cpp -- the host twins of row_vectors_kernel, score_rows_kernel, row_stats_kernel, col_stats_kernel, assign_kernel, nearest_kernel and label_sums_kernel (packed_host.hpp).
#include "packed_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/tkspmv.h"
#include "quantise.hpp"

namespace tkspmv {

// The one prologue of the twins: fp32 values only, a complete matrix, and the view of its stream. `what` opens the refusal's text.
static int open_f32_stream(const PackedMatrix &pm, const char *what, HostRowView &V, std::string &err) {
    if (pm.precision != Precision::F32 && pm.precision != Precision::F32C12) {
        err = std::string(what) + " fp32 packet streams only (TKSPMV_F32)";
        return TKSPMV_ERR_UNSUPPORTED;
    }
    if (pm.packets.size() != pm.stream_bytes() || pm.pkt_row.size() != pm.n_packets) {
        err = "the packed matrix is incomplete";
        return TKSPMV_ERR_INVALID;
    }
    V = HostRowView{pm.packets.data(), pm.pkt_row.data(), pm.part_first.data(), pm.part_count.data(), pm.packet_bytes, pm.packet_entries, pm.C,
                    pm.precision == Precision::F32C12};
    return TKSPMV_OK;
}

// Entries of row r and, where it has any, its run. 0: a placeholder, a row beyond the last stored one, or no packets at all.
static uint32_t locate_entries(const PackedMatrix &pm, const HostRowView &V, uint32_t r, RowRun &run) {
    if (!locate_row(V, r, pm.n_packets, (uint32_t)pm.part_first.size(), V.PE, run)) return 0u;
    return row_run_entries(run, V.PE, V.word(run.first_pkt, run.first_slot));
}

// The score of one located row from its own packets: reduce_core (kernels/packet_math.hpp) restated lane by lane, what
// score_rows_kernel (kernels/score_rows.hpp) runs on the device. Per packet of the run: products inside the run, +0.0f outside; every
// slot's own ROW_END mask; the carry +0.0f in front of the first packet. Every sum and product is a separately rounded fp32 operation
// (-ffp-contract=off), in the kernel's order. product(value, column word) is the product of one slot inside the run: v * x[col] for a
// score, a function of v alone for a row statistic (row_stats_kernel, kernels/row_stats.hpp).
template <class Product>
static float reduce_located_row(const HostRowView &V, const RowRun &run, Product product) {
    const uint32_t C = V.C;
    float carry = 0.0f, score = 0.0f;
    for (uint32_t pk = run.first_pkt; pk <= run.last_pkt; ++pk) {
        float s[64][8], head[64], tail[64], vv[64], t[64];
        bool end[64][8];
        uint64_t H = 0;  // lanes that hold a row end
        for (uint32_t l = 0; l < 64u; ++l) {
            float p[8];
            for (uint32_t j = 0; j < C; ++j) {
                const uint32_t ss = l * C + j;
                const uint16_t w = V.word(pk, ss);
                const bool inside = (pk > run.first_pkt || ss >= run.first_slot) && (pk < run.last_pkt || ss <= run.last_slot);
                p[j] = inside ? product(V.value(pk, ss), w) : 0.0f;
                end[l][j] = (w & COLW_ROW_END) != 0;
                if (end[l][j]) H |= 1ull << l;
            }
            if (l == 0u) p[0] = p[0] + carry;
            s[l][0] = p[0];
            for (uint32_t j = 1; j < C; ++j) s[l][j] = (end[l][j - 1] ? 0.0f : s[l][j - 1]) + p[j];
            head[l] = s[l][C - 1];
            for (uint32_t j = C - 1; j-- > 0u;)
                if (end[l][j]) head[l] = s[l][j];
            tail[l] = end[l][C - 1] ? 0.0f : s[l][C - 1];
        }
        // the clipped scan: the lane masks of reduce_core, bit for bit
        const uint64_t M1 = ~H, M2 = M1 & (M1 << 1), M4 = M2 & (M2 << 2), M8 = M4 & (M4 << 4);
        const uint64_t X16 = M1 & 0xFFFF0000FFFF0000ull, P16 = X16 & ~(X16 + 0x0001000000010000ull);
        const uint32_t Z32 = (uint32_t)(M1 >> 32);
        const uint64_t P32 = (uint64_t)(Z32 & ~(Z32 + 1u)) << 32;
        for (uint32_t l = 0; l < 64u; ++l) vv[l] = tail[l];
        const uint64_t masks[4] = {M1, M2, M4, M8};
        for (uint32_t step = 0; step < 4u; ++step) {  // row_shr:1, 2, 4, 8 inside each row of 16 lanes; a lane without a source adds +0.0f
            const uint32_t d = 1u << step;
            for (uint32_t l = 0; l < 64u; ++l) t[l] = vv[l] + ((l & 15u) >= d ? vv[l - d] : 0.0f);
            for (uint32_t l = 0; l < 64u; ++l)
                if ((masks[step] >> l) & 1u) vv[l] = t[l];
        }
        for (uint32_t l = 0; l < 64u; ++l) t[l] = ((l >> 4) & 1u) ? vv[(l & ~15u) - 1u] + vv[l] : vv[l];  // row_bcast:15: lane 15 -> row 1, lane 47 -> row 3
        for (uint32_t l = 0; l < 64u; ++l)
            if ((P16 >> l) & 1u) vv[l] = t[l];
        for (uint32_t l = 32; l < 64u; ++l) t[l] = vv[31] + vv[l];  // row_bcast:31: lane 31 -> rows 2 and 3
        for (uint32_t l = 32; l < 64u; ++l)
            if ((P32 >> l) & 1u) vv[l] = t[l];
        carry = vv[63];
        if (pk == run.last_pkt) {  // expand(): the first row end of a lane yields S, later ones their own s[j]
            const uint32_t l = run.last_slot / C, j = run.last_slot % C;
            bool earlier = false;
            for (uint32_t i = 0; i < j; ++i) earlier = earlier || end[l][i];
            const float S = (l == 0u ? 0.0f : vv[l - 1u]) + head[l];
            score = earlier ? s[l][j] : S;
        }
    }
    return score;
}
static float score_located_row(const HostRowView &V, const RowRun &run, const float *x) {
    return reduce_located_row(V, run, [x](float v, uint16_t w) { return v * x[w >> COLW_COL_SHIFT]; });
}
// The cosine weight of a row whose squares sum to l2sq (inv_l2_of, kernels/row_stats.hpp): two separately rounded fp32 operations;
// +0.0f where the sum is 0, +inf or NaN.
static float inv_l2_of(float l2sq) {
    const float w = 1.0f / std::sqrt(l2sq);
    return (l2sq > 0.0f && l2sq < std::numeric_limits<float>::infinity()) ? w : 0.0f;
}

// The order keys of the column extremes (order_key / key_to_float, kernels/common.hpp, on bit patterns): monotone in the float's
// total order, 0 the key of no float.
static uint32_t order_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
static uint32_t key_to_float(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key; }

int packed_get_row(const PackedMatrix &pm, uint32_t row, uint32_t *col, float *val, uint32_t capacity, uint32_t *n, std::string &err) {
    if (row >= pm.rows) {
        err = "row out of range (>= rows)";
        return TKSPMV_ERR_INVALID;
    }
    HostRowView V;
    if (const int st = open_f32_stream(pm, "rows are looked up in", V, err); st != TKSPMV_OK) return st;
    RowRun run{0u, 0u, 0u, 0u};
    *n = locate_entries(pm, V, row, run);
    if (*n == 0u) return TKSPMV_OK;
    uint32_t out = 0u;
    for (uint32_t pk = run.first_pkt; pk <= run.last_pkt && out < capacity; ++pk) {
        const uint32_t s0 = pk == run.first_pkt ? run.first_slot : 0u, s1 = pk == run.last_pkt ? run.last_slot : V.PE - 1u;
        for (uint32_t ss = s0; ss <= s1 && out < capacity; ++ss, ++out) {
            col[out] = (uint32_t)(V.word(pk, ss) >> COLW_COL_SHIFT);
            val[out] = V.value(pk, ss);
        }
    }
    return TKSPMV_OK;
}

int packed_score_rows(const PackedMatrix &pm, const float *x, const uint32_t *rows, int32_t n_rows, float *scores, std::string &err) {
    for (int32_t i = 0; i < n_rows; ++i)
        if (rows[i] >= pm.rows) {
            err = "row out of range (>= rows)";
            return TKSPMV_ERR_INVALID;
        }
    HostRowView V;
    if (const int st = open_f32_stream(pm, "rows are scored in", V, err); st != TKSPMV_OK) return st;
    for (int32_t i = 0; i < n_rows; ++i) {
        RowRun run{0u, 0u, 0u, 0u};
        scores[i] = locate_entries(pm, V, rows[i], run) ? score_located_row(V, run, x) : 0.0f;  // a row without entries: +0.0f
    }
    return TKSPMV_OK;
}

int packed_row_stats(const PackedMatrix &pm, int32_t kind, float *out, std::string &err) {
    HostRowView V;
    if (const int st = open_f32_stream(pm, "row statistics are taken from", V, err); st != TKSPMV_OK) return st;
    for (uint32_t r = 0; r < pm.rows; ++r) {
        RowRun run{0u, 0u, 0u, 0u};
        out[r] = 0.0f;  // a row without entries: a placeholder, or no packets at all
        if (locate_entries(pm, V, r, run) == 0u) continue;
        switch (kind) {
            case TKSPMV_ROW_NNZ: out[r] = reduce_located_row(V, run, [](float, uint16_t) { return 1.0f; }); break;
            case TKSPMV_ROW_L1: out[r] = reduce_located_row(V, run, [](float v, uint16_t) { return std::fabs(v); }); break;
            case TKSPMV_ROW_L2SQ: out[r] = reduce_located_row(V, run, [](float v, uint16_t) { return v * v; }); break;
            default: out[r] = inv_l2_of(reduce_located_row(V, run, [](float v, uint16_t) { return v * v; })); break;
        }
    }
    return TKSPMV_OK;
}

// assign_kernel (kernels/assign.hpp) restated: packed_nearest's lists of one entry without a mask -- the first vector kept, a later one
// only where it scores strictly more; a row without entries: label 0, +0.0f. best = NULL: the scores go to an array of this call.
int packed_assign(const PackedMatrix &pm, const float *xs, int32_t count, uint32_t *labels, float *best, std::string &err) {
    std::vector<float> scores(best ? 0u : pm.rows);
    return packed_nearest(pm, xs, count, 1, nullptr, labels, best ? best : scores.data(), err);
}

// nearest_kernel (kernels/nearest.hpp) restated row by row: the row's score against every vector in turn -- packed_score_rows' value --,
// each placed behind every kept entry that scores at least as much (ties go to the smaller index), the first n kept. Entries beyond
// count: (TKSPMV_NEAREST_NONE, -inf). A row without entries scores +0.0f throughout; a row outside the mask is padding throughout.
int packed_nearest(const PackedMatrix &pm, const float *xs, int32_t count, int32_t n, const uint32_t *mask, uint32_t *labels, float *scores, std::string &err) {
    HostRowView V;
    if (const int st = open_f32_stream(pm, "rows are assigned in", V, err); st != TKSPMV_OK) return st;
    const float none = -std::numeric_limits<float>::infinity();
    for (uint32_t r = 0; r < pm.rows; ++r) {
        uint32_t *const lb = labels + (size_t)r * (size_t)n;
        float *const sc = scores + (size_t)r * (size_t)n;
        for (int32_t j = 0; j < n; ++j) {
            lb[j] = TKSPMV_NEAREST_NONE;
            sc[j] = none;
        }
        if (mask && ((mask[r >> 5] >> (r & 31u)) & 1u) == 0u) continue;
        RowRun run{0u, 0u, 0u, 0u};
        const bool stored = locate_entries(pm, V, r, run) != 0u;
        int32_t len = 0;  // entries kept so far
        for (int32_t q = 0; q < count; ++q) {
            const float s = stored ? score_located_row(V, run, xs + (size_t)q * pm.cols) : 0.0f;
            int32_t at = len;  // behind every entry with a score >= s
            while (at > 0 && s > sc[at - 1]) --at;
            if (at >= n) continue;
            for (int32_t j = std::min(len, n - 1); j > at; --j) {
                sc[j] = sc[j - 1];
                lb[j] = lb[j - 1];
            }
            sc[at] = s;
            lb[at] = (uint32_t)q;
            if (len < n) ++len;
        }
    }
    return TKSPMV_OK;
}

// col_stats_kernel (kernels/col_stats.hpp) restated as a walk over the stream, from what the device has: the packets, pkt_row and the
// partition table. Per partition: its last row end is looked for from its last packet backwards; the slots up to it, in stream order,
// are its entries -- what lies behind is padding --, a SKIP slot is the placeholder of an empty row, and the row of a slot is the row of
// the partition's first packet plus the row ends in front of it. MAX / MIN compare order keys; MIN is the MAX of the negated values.
int packed_col_stats(const PackedMatrix &pm, int32_t kind, const uint32_t *mask, void *out, std::string &err) {
    HostRowView V;
    if (const int st = open_f32_stream(pm, "column statistics are taken from", V, err); st != TKSPMV_OK) return st;
    const uint32_t negate = kind == TKSPMV_COL_MIN ? 0x80000000u : 0u;
    std::vector<uint32_t> acc(pm.cols, 0u);  // counts, or order keys (0: no counted entry)
    for (size_t q = 0; q < pm.part_first.size(); ++q) {
        const uint32_t f0 = pm.part_first[q];
        uint32_t n = 0u, last_slot = 0u;
        for (uint32_t k = pm.part_count[q]; k > 0u; --k)
            if (V.last_end(f0 + k - 1u, last_slot)) {
                n = k;
                break;
            }
        uint32_t r = n ? pm.pkt_row[f0] : 0u;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t lim = k + 1u == n ? last_slot : V.PE - 1u;
            for (uint32_t ss = 0; ss <= lim; ++ss) {
                const uint16_t w = V.word(f0 + k, ss);
                const uint32_t c = (uint32_t)(w >> COLW_COL_SHIFT);
                const bool allowed = !mask || (r < pm.rows && ((mask[r >> 5] >> (r & 31u)) & 1u));
                if (!(w & COLW_SKIP) && allowed && c < pm.cols) {
                    if (kind == TKSPMV_COL_NNZ) {
                        ++acc[c];
                    } else {
                        uint32_t bits;
                        const float v = V.value(f0 + k, ss);
                        std::memcpy(&bits, &v, 4);
                        acc[c] = std::max(acc[c], order_key(bits ^ negate));
                    }
                }
                if (w & COLW_ROW_END) ++r;
            }
        }
    }
    uint32_t *const o = static_cast<uint32_t *>(out);
    for (uint32_t c = 0; c < pm.cols; ++c)  // key 0: -inf; then the negation of MIN undone
        o[c] = kind == TKSPMV_COL_NNZ ? acc[c] : ((acc[c] == 0u ? 0xFF800000u : key_to_float(acc[c])) ^ negate);
    return TKSPMV_OK;
}

// label_sums_close_kernel (kernels/label_sums.hpp) restated: FLOAT's value is ldexp of the int64 rounded to fp32 (nearest even); UNIT
// forms the 64 partials of the squares in double -- partial l: the columns l, l + 64, ... ascending --, adds them in the order 0 .. 63,
// and scales by inv_l2_of; a bin whose weight is 0 is not written.
void sums_close_host(const int64_t *sums, uint32_t n_bins, uint32_t cols, int32_t quantum_exp, int32_t mode, float *out) {
    for (uint32_t b = 0; b < n_bins; ++b) {
        const int64_t *const s = sums + (size_t)b * cols;
        float *const o = out + (size_t)b * cols;
        if (mode != TKSPMV_SUMS_UNIT) {
            for (uint32_t c = 0; c < cols; ++c) o[c] = std::ldexp((float)s[c], quantum_exp);
            continue;
        }
        double part[64] = {};
        for (uint32_t c = 0; c < cols; ++c) {
            const double f = (double)std::ldexp((float)s[c], quantum_exp);
            part[c & 63u] += f * f;
        }
        double n2 = 0.0;
        for (int l = 0; l < 64; ++l) n2 += part[l];
        const float w = inv_l2_of((float)n2);
        if (w == 0.0f) continue;
        for (uint32_t c = 0; c < cols; ++c) o[c] = std::ldexp((float)s[c], quantum_exp) * w;
    }
}

// label_sums_kernel (kernels/label_sums.hpp) restated row by row: every row located in the stream (locate_row), the entries of its
// run -- a placeholder has none, and padding belongs to no row -- quantised and added to the word of the row's label and their column.
int packed_label_sums(const PackedMatrix &pm, const uint32_t *labels, uint32_t n_bins, int32_t quantum_exp, int32_t mode, int64_t *sums, float *out, std::string &err) {
    HostRowView V;
    if (const int st = open_f32_stream(pm, "label sums are taken from", V, err); st != TKSPMV_OK) return st;
    std::vector<uint64_t> acc((size_t)n_bins * pm.cols, 0ull);  // (unsigned: the additions wrap like the device's)
    for (uint32_t r = 0; r < pm.rows; ++r) {
        RowRun run{0u, 0u, 0u, 0u};
        if (labels[r] >= n_bins || locate_entries(pm, V, r, run) == 0u) continue;
        uint64_t *const a = acc.data() + (size_t)labels[r] * pm.cols;
        for (uint32_t pk = run.first_pkt; pk <= run.last_pkt; ++pk) {
            const uint32_t s0 = pk == run.first_pkt ? run.first_slot : 0u, s1 = pk == run.last_pkt ? run.last_slot : V.PE - 1u;
            for (uint32_t ss = s0; ss <= s1; ++ss) {
                const uint32_t c = (uint32_t)(V.word(pk, ss) >> COLW_COL_SHIFT);
                const float v = V.value(pk, ss);
                uint32_t bits;
                std::memcpy(&bits, &v, 4);
                if (c < pm.cols) a[c] += (uint64_t)quantise(bits, quantum_exp);
            }
        }
    }
    if (sums) std::memcpy(sums, acc.data(), acc.size() * 8);
    if (mode != TKSPMV_SUMS_RAW) sums_close_host(reinterpret_cast<const int64_t *>(acc.data()), n_bins, pm.cols, quantum_exp, mode, out);
    return TKSPMV_OK;
}

int packed_sums_exponent(const PackedMatrix &pm, int32_t *quantum_exp, std::string &err) {
    std::vector<uint32_t> nnz(pm.cols), hi(pm.cols), lo(pm.cols);
    if (const int st = packed_col_stats(pm, TKSPMV_COL_NNZ, nullptr, nnz.data(), err); st != TKSPMV_OK) return st;
    if (const int st = packed_col_stats(pm, TKSPMV_COL_MAX, nullptr, hi.data(), err); st != TKSPMV_OK) return st;
    if (const int st = packed_col_stats(pm, TKSPMV_COL_MIN, nullptr, lo.data(), err); st != TKSPMV_OK) return st;
    *quantum_exp = sums_exponent_of_columns(nnz.data(), hi.data(), lo.data(), pm.cols);
    return TKSPMV_OK;
}

}  // namespace tkspmv
