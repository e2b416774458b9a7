// row_lookup.hpp -- where one row lives in the wave-BSCSR packet stream (wbscsr.hpp): the lookup behind
// tkspmv_packed_get_row (host, packed_host.cpp) and row_vectors_kernel (device, kernels/row_vectors.hpp). One definition for both,
// as slot_to_index is for the packers: the host decoder and the kernel cannot drift apart.
//
// The stream stores no row ids per entry and no row pointers; what it has is pkt_row[p], the row of packet p's FIRST entry.
// The stream is packed partition by partition in row order and every packet has a real entry (or the placeholder of an empty
// row) at slot 0, so pkt_row is non-decreasing over the whole stream and can be bisected:
//   * row r ENDS in the last packet p with pkt_row[p] <= r, at that packet's (r - pkt_row[p] + 1)-th ROW_END. A packet with
//     fewer row ends than that: r lies beyond the last stored row (trailing empty rows have no packets at all).
//   * if that is not the packet's first row end, the row starts right behind the one before it, in the same packet;
//   * else the row is the one of the packet's first entry. It starts in the first packet f with pkt_row[f] == r (the packets
//     in between belong to it whole) at slot 0, or behind the last ROW_END of packet f - 1 -- unless f opens a partition:
//     a row never crosses a partition, and the tail of a partition's last packet is zero padding (column word 0, value 0, no
//     flags) that looks exactly like the head of the next row.
//   * a placeholder entry (SKIP) is a whole row: "exists, no entries".
#pragma once
#include <cstdint>

#include "wbscsr.hpp"

namespace tkspmv {

// The entries of one row: stream slots (0 .. PE-1, the order of the matrix; slot_to_index() gives the position in the packet)
// [first_slot of first_pkt, last_slot of last_pkt], every packet in between whole.
struct RowRun {
    uint32_t first_pkt, first_slot, last_pkt, last_slot;
};

// Column word of stream slot ss of a packet with fp32 values: 16-bit words behind the values (Precision::F32, C = 4 or 8, two
// planes at C = 8), or the split 12-bit words of Precision::F32C12 (C = 4).
TKSPMV_HD inline uint16_t f32_colword_at(const uint8_t *pkt, uint32_t PE, uint32_t C, bool c12, uint32_t ss) {
    const uint32_t s = slot_to_index(ss, C);
    if (c12) return colw12s_load(pkt + (size_t)PE * 4u, s);
    uint16_t cw;
    __builtin_memcpy(&cw, pkt + (size_t)PE * 4u + (size_t)s * 2u, 2);
    return cw;
}
TKSPMV_HD inline float f32_value_at(const uint8_t *pkt, uint32_t C, uint32_t ss) {
    float v;
    __builtin_memcpy(&v, pkt + (size_t)slot_to_index(ss, C) * 4u, 4);
    return v;
}

// Number of leading elements <= v (strict: < v) of the non-decreasing sequence t(0) .. t(n-1).
template <class Table>
TKSPMV_HD inline uint32_t count_le(const Table &t, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (t(mid) <= v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
template <class Table>
TKSPMV_HD inline uint32_t count_lt(const Table &t, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (t(mid) < v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// Locates local row r. View is how the caller reads the stream -- a loop over slots on the host, a wave on the device:
//   uint32_t pkt_row(p), part_first(q), part_count(q)          the side tables
//   bool kth_end(p, k, slot)   stream slot of the k-th (k >= 1) ROW_END of packet p; false: the packet has fewer
//   bool last_end(p, slot)     ... of its last ROW_END; false: it has none
// Returns false when the row has no packets (beyond the last stored row, or an empty stream). A row that exists without
// entries comes back as the one slot of its placeholder: row_run_entries() tells.
template <class View>
TKSPMV_HD inline bool locate_row(const View &V, uint32_t r, uint32_t n_packets, uint32_t n_parts, uint32_t PE, RowRun &run) {
    const auto rows_of = [&V](uint32_t p) { return V.pkt_row(p); };
    const uint32_t n_le = count_le(rows_of, n_packets, r);
    if (n_le == 0u) return false;
    const uint32_t pe = n_le - 1u;
    const uint32_t k = r - V.pkt_row(pe) + 1u;
    uint32_t s_end = 0u, s_prev = 0u;
    if (!V.kth_end(pe, k, s_end)) return false;
    run.last_pkt = pe;
    run.last_slot = s_end;
    run.first_pkt = pe;
    run.first_slot = 0u;
    if (k >= 2u) {  // starts behind the row end before it, in the same packet
        (void)V.kth_end(pe, k - 1u, s_prev);
        run.first_slot = s_prev + 1u;
        return true;
    }
    const uint32_t pf = count_lt(rows_of, n_packets, r);  // (<= pe: pkt_row[pe] == r)
    run.first_pkt = pf;
    if (pf == 0u) return true;
    // does pf open a partition? (the partition that holds it: the last one with part_first <= pf, pf inside its packets)
    const auto firsts = [&V](uint32_t q) { return V.part_first(q); };
    const uint32_t q = count_le(firsts, n_parts, pf);
    if (q == 0u || V.part_first(q - 1u) == pf || pf - V.part_first(q - 1u) >= V.part_count(q - 1u)) return true;
    // the packet before holds rows below r: its last ROW_END is theirs, what follows it is the head of r
    if (V.last_end(pf - 1u, s_prev) && s_prev + 1u < PE) {
        run.first_pkt = pf - 1u;
        run.first_slot = s_prev + 1u;
    }
    return true;
}

// Entries of a located row; first_word = the column word of its first slot (a placeholder: the row has none).
TKSPMV_HD inline uint32_t row_run_entries(const RowRun &run, uint32_t PE, uint16_t first_word) {
    if (first_word & COLW_SKIP) return 0u;
    return (run.last_pkt - run.first_pkt) * PE + run.last_slot + 1u - run.first_slot;
}

}  // namespace tkspmv
