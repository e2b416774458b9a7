// packed_host.hpp -- the host twins of six kernels over a packed fp32 stream (wbscsr.hpp), behind tkspmv_packed_get_row,
// tkspmv_packed_score_rows, tkspmv_packed_row_stats, tkspmv_packed_col_stats, tkspmv_packed_assign, tkspmv_packed_nearest and tkspmv_packed_label_sums (c_api.cpp). Plain C++ over a PackedMatrix, no GPU:
// what they return agrees with the device bit for bit, and the host tests compare them with models that share nothing with them.
#pragma once
#include <cstdint>
#include <string>

#include "row_lookup.hpp"

namespace tkspmv {

// The host's view of a packed fp32 stream for locate_row (row_lookup.hpp): plain loops over the slots of a packet.
struct HostRowView {
    const uint8_t *packets;
    const uint32_t *pkt_row_, *part_first_, *part_count_;
    uint32_t packet_bytes, PE, C;
    bool c12;
    uint32_t pkt_row(uint32_t p) const { return pkt_row_[p]; }
    uint32_t part_first(uint32_t q) const { return part_first_[q]; }
    uint32_t part_count(uint32_t q) const { return part_count_[q]; }
    uint16_t word(uint32_t p, uint32_t ss) const { return f32_colword_at(packets + (size_t)p * packet_bytes, PE, C, c12, ss); }
    float value(uint32_t p, uint32_t ss) const { return f32_value_at(packets + (size_t)p * packet_bytes, C, ss); }
    bool kth_end(uint32_t p, uint32_t k, uint32_t &slot) const {
        for (uint32_t ss = 0; ss < PE; ++ss)
            if ((word(p, ss) & COLW_ROW_END) && --k == 0u) {
                slot = ss;
                return true;
            }
        return false;
    }
    bool last_end(uint32_t p, uint32_t &slot) const {
        for (uint32_t ss = PE; ss-- > 0u;)
            if (word(p, ss) & COLW_ROW_END) {
                slot = ss;
                return true;
            }
        return false;
    }
};

// Each returns a TKSPMV_* status and fills err when it is not TKSPMV_OK: TKSPMV_ERR_UNSUPPORTED for a stream whose values are not
// fp32, TKSPMV_ERR_INVALID for an incomplete matrix or a row >= rows. Pointers and `kind` are the caller's to check (c_api.cpp does);
// the contracts are those of the tkspmv_packed_* functions of include/tkspmv.h.
int packed_get_row(const PackedMatrix &pm, uint32_t row, uint32_t *col, float *val, uint32_t capacity, uint32_t *n, std::string &err);
int packed_score_rows(const PackedMatrix &pm, const float *x, const uint32_t *rows, int32_t n_rows, float *scores, std::string &err);
int packed_row_stats(const PackedMatrix &pm, int32_t kind, float *out, std::string &err);
int packed_col_stats(const PackedMatrix &pm, int32_t kind, const uint32_t *mask, void *out, std::string &err);
int packed_assign(const PackedMatrix &pm, const float *xs, int32_t count, uint32_t *labels, float *best, std::string &err);
// nearest_fill_kernel and nearest_kernel (kernels/nearest.hpp): every row's n best vectors in order, under an optional allow-mask.
int packed_nearest(const PackedMatrix &pm, const float *xs, int32_t count, int32_t n, const uint32_t *mask, uint32_t *labels, float *scores, std::string &err);
// label_sums_kernel and label_sums_close_kernel (kernels/label_sums.hpp): the int64 sums of every label and column, the default
// exponent, and the closing rule alone (mode TKSPMV_SUMS_FLOAT / _UNIT; UNIT leaves a bin without a norm unwritten).
int packed_label_sums(const PackedMatrix &pm, const uint32_t *labels, uint32_t n_bins, int32_t quantum_exp, int32_t mode, int64_t *sums, float *out, std::string &err);
int packed_sums_exponent(const PackedMatrix &pm, int32_t *quantum_exp, std::string &err);
void sums_close_host(const int64_t *sums, uint32_t n_bins, uint32_t cols, int32_t quantum_exp, int32_t mode, float *out);

}  // namespace tkspmv
