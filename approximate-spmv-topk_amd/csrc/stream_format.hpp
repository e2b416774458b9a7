// stream_format.hpp -- which packet streams exist and what a kernel is instantiated with for each: the one place that turns
// (descriptor precision, stream value type, packet entries, columns) into the kernels' template arguments. Host-only, plain C++:
// the kernels include it for the names, engine.hip for the table and the list its dispatch is generated from.
#pragma once
#include <cstdint>

#include "../../include/tkspmv.h"
#include "wbscsr.hpp"

namespace tkspmv {

// QM, the kernels' arithmetic mode (template parameter, an int): the stream's Precision except for the wide mode, which reads the
// Q1.7 stream. What each mode computes is described in kernels/common.hpp.
constexpr int QM_F32 = 0, QM_Q17 = 1, QM_Q17_WIDE = 2, QM_F16 = 3, QM_FIXED = 4, QM_Q17_F32 = 5, QM_FIXED20 = 6, QM_F32C12 = 7, QM_FIXED26 = 8, QM_F32E5 = 9;
static_assert(QM_F32 == (int)Precision::F32 && QM_Q17 == (int)Precision::Q1_7 && QM_F16 == (int)Precision::F16 && QM_FIXED == (int)Precision::FIXED &&
                  QM_Q17_F32 == (int)Precision::Q1_7_RND && QM_FIXED20 == (int)Precision::FIXED20 && QM_F32C12 == (int)Precision::F32C12 &&
                  QM_FIXED26 == (int)Precision::FIXED26 && QM_F32E5 == (int)Precision::F32E5,
              "QM is the numeric value of the stream's Precision (QM_Q17_WIDE aside: it has no stream of its own)");

// VT, how a lane's share of a packet is laid out (Pkt, load_packet): C fp32 words + 16-bit column words; Q1.7 bytes four to a dword;
// fp16 values two to a dword; FIXED20's packed dwords; fp32 words + the split 12-bit column plane; Q1.7 bytes + back-to-back 12-bit
// column words (the row-per-lane chunks of multi_kernel only); FIXED26's four dwords + one; F32E5's four dwords + one.
constexpr int VT_F32 = 0, VT_Q17 = 1, VT_F16 = 2, VT_FIXED20 = 3, VT_F32C12 = 4, VT_Q17C12 = 5, VT_FIXED26 = 6, VT_F32E5 = 7;
constexpr int value_type_of(int QM) {  // QM_FIXED: one u32 per value, loaded like fp32
    return QM == QM_F32E5 ? VT_F32E5 : QM == QM_FIXED26 ? VT_FIXED26 : QM == QM_F32C12 ? VT_F32C12 : QM == QM_FIXED20 ? VT_FIXED20 : QM == QM_F16 ? VT_F16
           : (QM == QM_Q17 || QM == QM_Q17_WIDE || QM == QM_Q17_F32) ? VT_Q17 : VT_F32;
}

// What a streaming kernel is instantiated with: entries per lane, the tier of x in LDS, the arithmetic mode. c == 0: no format.
struct StreamFormat { int c, xcols, qm; };
constexpr int xcols_tier(uint32_t cols) { return cols <= 1024u ? 1024 : (cols <= 4096u ? 4096 : 16384); }

// Every format, once: X(C, XCOLS, QM). The bit-packed and 12-bit-column streams and 8 entries per lane exist at 1024 columns only.
// (QM_F32E5 is not in the list: no packer writes that stream and no descriptor asks for it -- the engine re-encodes its F32C12 stream
//  for the batch kernel where the values allow, and instantiates that kernel by hand: engine.hip compact_stream / choose_kernels.)
#define TKSPMV_FORMAT_TIERS(X, QM) X(4, 1024, QM) X(4, 4096, QM) X(4, 16384, QM)
#define TKSPMV_STREAM_FORMATS(X)                                                                                             \
    X(4, 1024, QM_F32C12) X(8, 1024, QM_F32) X(4, 1024, QM_FIXED20) X(4, 1024, QM_FIXED26)                                   \
    TKSPMV_FORMAT_TIERS(X, QM_F32) TKSPMV_FORMAT_TIERS(X, QM_Q17) TKSPMV_FORMAT_TIERS(X, QM_Q17_WIDE) TKSPMV_FORMAT_TIERS(X, QM_F16) \
    TKSPMV_FORMAT_TIERS(X, QM_FIXED) TKSPMV_FORMAT_TIERS(X, QM_Q17_F32)

constexpr bool is_fp32(StreamFormat f) { return f.qm == QM_F32 || f.qm == QM_F32C12; }  // filtered, range and row-vector kernels
constexpr bool is_batchable(StreamFormat f) { return f.xcols == 1024; }  // batch_kernel holds x twice in LDS: larger x, and two workgroups no longer fit a CU
constexpr bool has_tracing_twins(StreamFormat f) { return f.c == 4 && f.xcols == 1024 && is_fp32(f); }  // the DBG instantiations
constexpr bool has_single_kernel(StreamFormat f) { return has_tracing_twins(f); }  // single_kernel is built for the same two formats

// The format of an engine's packet stream, from the descriptor's precision (tkspmv_precision), the stream's value type, its entries
// per packet and the matrix's columns. Nothing else decides it: no option, no device property.
inline StreamFormat stream_format_of(int32_t api_precision, Precision stream, uint32_t packet_entries, uint32_t cols) {
    struct Row { int32_t api; Precision stream; uint32_t entries; int qm; bool tiered; };  // tiered: built at 4096 and 16384 columns too
    static constexpr Row rows[] = {
        {TKSPMV_F32, Precision::F32C12, 256, QM_F32C12, false},
        {TKSPMV_F32, Precision::F32, 512, QM_F32, false},  // (8 entries per lane: creation rejects more than 1024 columns)
        {TKSPMV_F32, Precision::F32, 256, QM_F32, true},
        {TKSPMV_Q1_7, Precision::Q1_7, 256, QM_Q17, true},
        {TKSPMV_Q1_7_WIDE, Precision::Q1_7, 256, QM_Q17_WIDE, true},
        {TKSPMV_F16, Precision::F16, 256, QM_F16, true},
        {TKSPMV_FIXED, Precision::FIXED, 256, QM_FIXED, true},
        {TKSPMV_FIXED, Precision::FIXED20, 256, QM_FIXED20, false},
        {TKSPMV_FIXED, Precision::FIXED26, 256, QM_FIXED26, false},
        {TKSPMV_Q1_7_F32, Precision::Q1_7_RND, 256, QM_Q17_F32, true},
    };
    for (const Row &r : rows)
        if (r.api == api_precision && r.stream == stream && r.entries == packet_entries)
            return StreamFormat{(int)(r.entries / WAVE), r.tiered ? xcols_tier(cols) : 1024, r.qm};
    return StreamFormat{0, 0, 0};
}

}  // namespace tkspmv
