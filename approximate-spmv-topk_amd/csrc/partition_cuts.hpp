// partition_cuts.hpp -- the rule that cuts the row-sorted stream into wave partitions (wbscsr.hpp), ONCE, for the host packer
// (wbscsr.cpp) and the device packer's cuts_kernel (device_pack.hip).
//
// S[0 .. n_rows] are the prefix sums of the placeholder-expanded row lengths (an empty row counts one entry). A partition takes
// rows while their entries fit its capacity, at least one row (a row longer than the capacity gets a partition of its own).
//   * P = the partitions asked for, but never more than packets / min_packets;
//   * uniform cuts: every partition holds m packets, m grown from ceil(E / (P x PE)) until the cuts come to at most P;
//   * balanced cuts (round 5). Partitions of m packets each come to fewer than the P asked for whenever E / (P x PE) is not close
//     below an integer -- 125k rows of 20: 3229 partitions of 3 packets for 4064 waves --, and a batch kernel's workgroups then
//     stream 6 or 7 partitions each: the launch waits for the ones with 7 (4.62 against 4.99 us per query with all at 8 of 2-3
//     packets). Where the uniform cut misses P by more than 1/8 (option value 2: 1/32 -- tuning runs), the packets are dealt out
//     instead: B of them over P partitions, partition p taking floor((p + 1) B / P) - floor(p B / P), B grown from the lower bound
//     by 1/64 until the rows fit. Not below two packets per partition: 50k rows dealt out one packet per wave measure 3.88 against
//     3.66 us per query. (Measured: at 250k and 500k rows -- 3847 and 3824 uniform partitions, 94 % of the waves -- dealing out
//     gains nothing, 5.98 against 5.83 and 8.5-8.7 against 8.7: those keep the uniform table, from which the kernels derive a
//     wave's range without a load.)
// The callers differ in two things, passed in: first_above(S, lo, hi, target) = the smallest index f in (lo, hi] with
// S[f] > target, given S[lo] <= target < S[hi] (a bisection on the host, a 64-ary search by one wave on the device), and
// first_row(p, r), which records that partition p starts at row r (every pass overwrites the previous one's; the last pass stands).
#pragma once
#include <cstdint>

#include "wbscsr.hpp"

namespace tkspmv {

using EntrySum = unsigned long long;

struct PartitionCuts {
    uint32_t n_parts, packets_per_partition;
};

// The most partitions a stream of E entries is cut into (the size of the tables first_row writes).
TKSPMV_HD inline uint32_t partition_limit(EntrySum E, uint32_t PE, uint32_t P_hint, uint32_t min_packets) {
    const EntrySum max_parts = (E + PE - 1) / PE / min_packets;
    return (uint32_t)(P_hint < max_parts ? P_hint : (max_parts < 1 ? 1 : max_parts));
}

// One pass of greedy cuts: m packets per partition, or (B != 0) B packets dealt out over P. Returns the partitions it comes to, P + 1
// as soon as they are more than P.
template <class FirstAbove, class FirstRow>
TKSPMV_HD inline uint32_t cut_pass(const EntrySum *S, uint32_t n_rows, EntrySum PE, EntrySum m, EntrySum B, uint32_t P, FirstAbove first_above,
                                   FirstRow first_row) {
    uint32_t a = 0, parts = 0;
    while (a < n_rows) {
        if (parts == P) return P + 1u;
        first_row(parts, a);
        const EntrySum p = parts++;
        const EntrySum target = S[a] + PE * (B != 0 ? ((p + 1) * B) / P - (p * B) / P : m);
        // rows a .. b-1 with S[b] - S[a] <= capacity: b = (first index in (a, n] with S[idx] > target) - 1, or n
        uint32_t b = n_rows;
        if (S[n_rows] > target) {
            b = first_above(S, a, n_rows, target) - 1u;
            if (b <= a) b = a + 1u;
        }
        a = b;
    }
    return parts;
}

template <class FirstAbove, class FirstRow>
TKSPMV_HD inline PartitionCuts cut_partitions(const EntrySum *S, uint32_t n_rows, uint32_t PE, uint32_t P_hint, uint32_t min_packets,
                                              uint32_t balanced, FirstAbove first_above, FirstRow first_row) {
    const EntrySum E = S[n_rows], packets_lb = (E + PE - 1) / PE;
    const uint32_t P = partition_limit(E, PE, P_hint, min_packets);
    EntrySum m = (E + (EntrySum)P * PE - 1) / ((EntrySum)P * PE);
    if (m < 1) m = 1;
    uint32_t used;
    while ((used = cut_pass(S, n_rows, PE, m, 0, P, first_above, first_row)) > P) ++m;  // padding pushed the cuts over P: one more packet each
    if (balanced != 0u && P >= 2u && packets_lb >= 2ull * P &&
        (balanced == 2u ? (EntrySum)used * 32u < (EntrySum)P * 31u : (EntrySum)used * 8u < (EntrySum)P * 7u)) {
        EntrySum B = packets_lb > P ? packets_lb : P;
        while ((used = cut_pass(S, n_rows, PE, 0, B, P, first_above, first_row)) > P) B += B / 64 > 1 ? B / 64 : 1;
        m = (B + P - 1) / P;
    }
    return PartitionCuts{used, (uint32_t)m};
}

}  // namespace tkspmv
