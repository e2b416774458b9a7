// kernels/match_kernel.hpp -- match_kernel: allow-masks from boolean predicates over the rows' own columns (tkspmv_enqueue_match).
// Part of engine.hip (one translation unit: included there behind the other kernel headers; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"

namespace tkspmv {

// range_kernel's streaming loop over the COLUMN PLANE alone. A query is a clause table (one u32 per column: bit c set = the column
// belongs to clause c) and a predicate over the 32 clause bits; a row's word W is the OR of table[col] over its entries, and the row
// matches when (W & must) == must, (W & must_not) == 0 and popcount(W & should) >= min_should. Which columns a row has does not
// depend on its values, so the value plane of a packet never travels: the lane loads its column words (8 bytes at 4 entries per
// lane, 16 at 8), which carry the ROW_END / SKIP flags as well. The table is staged where range_kernel stages x -- at LDS offset 0,
// one word per column --, so an entry's table word is found by the address arithmetic of reduce_packet. Per packet: the segmented
// OR (or_packet, reduce_core with OR for ADD), then the lane's union U of everything a finished row of the lane can be made of; a
// packet in which no lane's U satisfies the predicate's monotone part (must, should) holds no matching row and is left without
// expanding -- must_not cannot be decided on a superset, so a predicate of must_not alone expands every packet.
// The mask is zeroed in front of the launch, so only words that hold a match are written. A wave's rows are consecutive over its
// partition: it collects the bits of the packets it expands in a ring of MATCH_RING words in LDS (its own: no other wave touches
// it) and writes the words out, a lane each, when the ring cannot take the next packet's rows and when the partition ends -- a few
// coalesced stores per partition instead of one per word as the rows move on (the two came out the same on the clock: DESIGN.md
// 3.17). A word goes out with a plain store, except for the first word the wave writes in a partition and the last, the only ones
// a neighbouring partition can share: partitions start and end on row boundaries -- the packers pad each to whole packets behind
// its last row (wbscsr.hpp, "WAVE PARTITIONS"; the carry of every streaming kernel starts at 0 for the same reason). Those two are
// OR-ed in atomically: at most two global atomics per partition and query whatever the predicate selects. One launch serves n_q
// queries; the table is handed over as range_kernel hands x over. No workgroup waits for another, and there is no timetable.
struct MatchParams {
    const uint8_t *replicas[16];  // the copies of the packet stream (cache-defeat mode); [0] alone otherwise
    uint32_t n_replicas;
    uint32_t q0;                  // number of this launch's first query within the call (picks the stream copies)
    uint32_t n_q;
    const uint32_t *clauses;      // query i of the launch: clauses + i * clause_stride words (0: one table for every query)
    uint64_t clause_stride;
    const tkspmv_match *preds;    // [n_q]
    const uint32_t *mask;         // FILT: query i's allow-mask at mask + i * mask_stride words
    uint32_t mask_stride, mask_words;
    uint32_t *out;                // query i's result at out + i * out_stride words (mask_words of them, zeroed in front of the launch)
    uint64_t out_stride;
    uint32_t *counts;             // [n_q] matching rows (zeroed in front of the launch), or NULL
    uint32_t args_tag;            // MATCH_ARGS_TAG: the kernel finds it where it expects R in its argument segment, or traps
};
constexpr uint32_t MATCH_ARGS_TAG = 0x3A7C4A65u;

constexpr uint32_t MATCH_RING = 64;  // words of a wave's ring (a lane each when it is written out): 2048 rows; a packet ends at most 64 x 8 rows, 17 words

template <int XCOLS>
struct MatchLds {
    uint32_t table[XCOLS];            // at LDS offset 0: (column word & 0xFFC) | tbase is the address of table[col]
    uint32_t ring[8][MATCH_RING];     // per wave: the mask words under construction, word w at [w % MATCH_RING]; zero when not in use
};

// A lane's share of a packet's column plane: Pkt's cw alone.
template <int C>
struct ColPkt {
    uint32_t cw[C / 2];  // QM_F32C12: the two dwords of the pair's 12-byte block that hold the lane's A and the pair's B (split_ab)
};
// load_packet_buf without the values, for 4 and for 8 entries per lane: one dwordx2 per plane of 4 entries at the lane's byte offset
// inside a packet (col_offset), which is the same for every packet. Loads beyond the resource's length return 0 (never requested: the
// kernel clamps to the last packet).
template <int C, int VT>
__device__ __forceinline__ uint32_t col_offset(uint32_t lane) {
    static_assert(VT == VT_F32 || (VT == VT_F32C12 && C == 4), "column plane of the fp32 packet streams");
    // (VT_F32C12: 12 bytes per pair of lanes, dwords 0-1 on the even lane, 1-2 on the odd one: load_packet)
    return VT == VT_F32C12 ? (uint32_t)C * 256u + (lane >> 1) * 12u + (lane & 1u) * 4u : (uint32_t)C * 256u + lane * 8u;
}
template <int C, int VT>
__device__ __forceinline__ void load_cols_buf(__amdgpu_buffer_rsrc_t rsrc, uint32_t packet_off, uint32_t coff, ColPkt<C> &o) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
        const u32x2 c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, coff + (uint32_t)q * 512u, packet_off, 2);  // (aux 2: non-temporal, like the flat form)
        o.cw[2 * q + 0] = c.x;
        o.cw[2 * q + 1] = c.y;
    }
}

// What the segmented OR leaves behind (Reduced, on clause words) and the packet's flag word (RowSums::fl, packet_flags' logic).
//   s[j] : OR over entry j's row segment inside the lane (lane 0's entry 0 includes the carry of the previous packet)
//   S    : the row word at the lane's FIRST row end = inclusive scan value of the lane below | the lane's head
//   m[j] : all ones where entry j ends a row
// Every finished row of the lane has its word in {S, s[1], ..., s[C-1]}.
template <int C>
struct MatchWords {
    uint32_t s[C];
    uint32_t S;
    uint32_t m[C];
    uint32_t fl;
};

template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {  // lanes without a source (or outside ROW_MASK) receive 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, BOUND);
}

// reduce_packet + reduce_core with OR where the scores have ADD (the same statements, on integers):
//   p_j = table[col_j];  p_0 |= carry on lane 0;  s_0 = p_0,  s_j = (end_{j-1} ? 0 : s_{j-1}) | p_j
//   tail = end_{C-1} ? 0 : s_{C-1};   head = s at the lane's first row end
//   vv = clipped Kogge-Stone scan of tail over the 64 lanes (never across a lane that holds a row end)
//   row word at the lane's first row end = vv[lane-1] | head, at its later row ends = s_j; carry' = vv[63]
// A placeholder of an empty row is a row of its own (it ends one, and the entry in front of it ended the row before), so what its
// column word points at reaches no other row; the padding behind a partition's last row reaches no row end at all.
template <int C, int QM>
__device__ __forceinline__ MatchWords<C> or_packet(const ColPkt<C> &cur, uint32_t &carry, const uint32_t tbase) {
    MatchWords<C> R;
    uint32_t p[C];
    bool has_end;
    if constexpr (QM == QM_F32C12) {
        static_assert(C == 4, "the split 12-bit plane is built for 4 entries per lane");
        uint32_t mask = 0xFFCu;
        asm("" : "+v"(mask));  // (kept in a register: v_and_or_b32 takes no literal)
        uint32_t A, B;
        split_ab(cur.cw[0], cur.cw[1], A, B);
        p[0] = lds_u32(and_or(A, mask, tbase));
        p[1] = lds_u32(and_or(A >> 10, mask, tbase));
        p[2] = lds_u32(and_or(A >> 20, mask, tbase));
        p[3] = lds_u32(and_or(B, mask, tbase));
        R.m[0] = bit_mask<12>(B);
        R.m[1] = bit_mask<13>(B);
        R.m[2] = bit_mask<14>(B);
        R.m[3] = bit_mask<15>(B);
        has_end = B > 0xFFFu;
        R.fl = (B >> 12) | ((A & 3u) << 8) | ((B & 3u) << 10);
    } else {
        uint32_t any = 0u, fl = 0u;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uint32_t word = cur.cw[j >> 1];
            p[j] = lds_u32(tbase + ((j & 1) ? ((word >> 16) & 0xFFFCu) : (word & 0xFFFCu)));  // LDS byte address of table[col]
            R.m[j] = (j & 1) ? bit_mask<16>(word) : bit_mask<0>(word);
            if ((j & 1) == 0) any |= word;
            const uint32_t w = word >> (16 * (j & 1));
            fl |= ((w & 1u) << j) | (((w >> 1) & 1u) << (8 + j));
        }
        has_end = (any & 0x00010001u) != 0u;
        R.fl = fl;
    }
    p[0] = __builtin_amdgcn_inverse_ballot_w64(1ull) ? (p[0] | carry) : p[0];  // lane 0 only
    R.s[0] = p[0];
#pragma unroll
    for (int j = 1; j < C; ++j) R.s[j] = (R.s[j - 1] & ~R.m[j - 1]) | p[j];
    uint32_t head = R.s[C - 1];
#pragma unroll
    for (int j = C - 2; j >= 0; --j) head = (R.s[j] & R.m[j]) | (head & ~R.m[j]);
    const uint32_t tail = R.s[C - 1] & ~R.m[C - 1];

    // The lane masks of reduce_core's clipped scan (see there).
    const uint64_t H = __ballot(has_end);
    const uint64_t M1 = ~H;
    const uint64_t M2 = M1 & (M1 << 1);
    const uint64_t M4 = M2 & (M2 << 2);
    const uint64_t M8 = M4 & (M4 << 4);
    const uint64_t X16 = M1 & 0xFFFF0000FFFF0000ull;
    const uint64_t P16 = X16 & ~(X16 + 0x0001000000010000ull);
    const uint32_t Z32 = (uint32_t)(M1 >> 32);
    const uint64_t P32 = (uint64_t)(Z32 & ~(Z32 + 1u)) << 32;

    uint32_t vv = tail, t;
    t = vv | dpp_u32<DPP_ROW_SHR1, 0xF, true>(vv);
    vv = __builtin_amdgcn_inverse_ballot_w64(M1) ? t : vv;
    t = vv | dpp_u32<DPP_ROW_SHR2, 0xF, true>(vv);
    vv = __builtin_amdgcn_inverse_ballot_w64(M2) ? t : vv;
    t = vv | dpp_u32<DPP_ROW_SHR4, 0xF, true>(vv);
    vv = __builtin_amdgcn_inverse_ballot_w64(M4) ? t : vv;
    t = vv | dpp_u32<DPP_ROW_SHR8, 0xF, true>(vv);
    vv = __builtin_amdgcn_inverse_ballot_w64(M8) ? t : vv;
    t = vv | dpp_u32<DPP_ROW_BCAST15, 0xA, false>(vv);  // lane 15 -> row 1, lane 47 -> row 3 (the other rows: | 0)
    vv = __builtin_amdgcn_inverse_ballot_w64(P16) ? t : vv;
    t = vv | dpp_u32<DPP_ROW_BCAST31, 0xC, false>(vv);  // lane 31 -> rows 2 and 3
    vv = __builtin_amdgcn_inverse_ballot_w64(P32) ? t : vv;
    R.S = dpp_u32<DPP_WAVE_SHR1, 0xF, true>(vv) | head;  // lane l-1's inclusive word; 0 for lane 0
    carry = (uint32_t)__builtin_amdgcn_readlane((int)vv, 63);
    return R;
}

// Scalar registers: the packet loop keeps the scan's lane masks, the buffer resource and the predicate's monotone part alive and has
// no room for more, so -- as facet_kernel does -- what only the rare paths need (the hand-over, a packet that is expanded, a flush, a
// further partition) is read from the kernel's argument segment where it is needed, and the table is requested through a buffer
// resource of cols words (no compare per word, whose lane masks would sit in scalar registers until the loads are issued).
template <int C, int XCOLS, int QM, bool FILT, int NBUF>
__global__ void __launch_bounds__(512, 4) match_kernel(const StreamParams P, const MatchParams R) {
    static_assert((QM == QM_F32 || QM == QM_F32C12) && (C == 4 || C == 8), "match_kernel: fp32 packet streams of 4 or 8 entries per lane");
    constexpr int VT = value_type_of(QM);
    constexpr uint32_t XPT = (uint32_t)XCOLS / 512u;  // words of the table per thread
    static_assert(XCOLS % 512 == 0, "the table is staged by 512 threads");
    static_assert(64u * C / 32u + 1u <= MATCH_RING, "a packet's rows fit the ring");
    __shared__ MatchLds<XCOLS> L;
    // (or_packet forms LDS addresses as (word & 0xFFC) | base: the table must sit on a 4 KiB boundary -- this object is the kernel's
    //  ONLY __shared__ block, so it starts at LDS address 0, and the table is its first member)
    static_assert(offsetof(MatchLds<XCOLS>, table) == 0, "the table must be the first member of the kernel's LDS block");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t part0 = wave * gridDim.x + blockIdx.x;
    const uint32_t tbase = lds_addr_of(L.table);
    uint32_t *const ring = L.ring[wave];
    ring[lane] = 0u;  // (the wave's own words: LDS executes a wave's instructions in order)
    // P and R as they lie in the kernel's argument segment (facet_kernel has the rule relied on and its guards: the static_assert on
    // padding, and the tag and two fields of either view compared at entry).
    typedef const char __attribute__((address_space(4))) *ArgBytes;
    typedef const MatchParams __attribute__((address_space(4))) *MatchArgs;
    typedef const StreamParams __attribute__((address_space(4))) *StreamArgs;
    static_assert(sizeof(StreamParams) % alignof(MatchParams) == 0, "R follows P without padding");
    auto arg_segment = [&]() __attribute__((always_inline)) {
        ArgBytes a = (ArgBytes)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(a));
        return a;
    };
    auto stream_args = [&]() __attribute__((always_inline)) { return (StreamArgs)arg_segment(); };
    auto match_args = [&]() __attribute__((always_inline)) { return (MatchArgs)(arg_segment() + sizeof(StreamParams)); };
    if (match_args()->args_tag != MATCH_ARGS_TAG || match_args()->n_q != R.n_q || stream_args()->n_parts != P.n_parts) __builtin_trap();

    // The wave's first partition. It is the same for every query and worked out again for each -- from the argument segment, so that
    // neither it nor what request_first derives from it is kept in scalar registers over the launch.
    auto first_partition = [&](uint32_t &f0, uint32_t &n) __attribute__((always_inline)) {
        const StreamArgs S = stream_args();
        f0 = 0u;
        n = 0u;
        if (part0 < S->n_parts) TKSPMV_PARTITION_RANGE(*S, part0, f0, n);
        f0 = __builtin_amdgcn_readfirstlane(f0);  // (wave-uniform by construction; said so: range_kernel)
        n = __builtin_amdgcn_readfirstlane(n);
    };

    ColPkt<C> buf[NBUF];
    const uint32_t coff = col_offset<C, VT>(lane);
    __amdgpu_buffer_rsrc_t rsrc = stream_resource(R.replicas[0], 0u);
    uint32_t req_off = 0u;
    // The first NBUF - 1 packets of partition [f0, f0 + n) in the stream copy of query qn (clamped to the last packet).
    auto request_first = [&](uint32_t qn, uint32_t f0, uint32_t n) __attribute__((always_inline)) {
        const MatchArgs A = match_args();
        rsrc = stream_resource(A->replicas[(A->q0 + qn) % A->n_replicas] + (size_t)f0 * P.packet_bytes, n * P.packet_bytes);
#pragma unroll
        for (int u = 0; u < NBUF - 1; ++u) {
            const uint32_t iu = ((uint32_t)u < n) ? (uint32_t)u : (n > 0u ? n - 1u : 0u);
            // (a resource of 0 bytes returns 0 and touches nothing: no branch around the loads of a wave without a partition)
            load_cols_buf<C, VT>(rsrc, iu * P.packet_bytes, coff, buf[u]);
        }
        req_off = (n > (uint32_t)(NBUF - 1) ? (uint32_t)(NBUF - 1) : (n > 0u ? n - 1u : 0u)) * P.packet_bytes;  // the next request's packet
    };
    // The table of query qn, XPT words per thread (issued back to back, ahead of the packets; a word beyond cols reads as 0)
    uint32_t tr[XPT];
    auto request_table = [&](uint32_t qn) __attribute__((always_inline)) {
        const MatchArgs A = match_args();
        const uint32_t cols = stream_args()->cols;
        const __amdgpu_buffer_rsrc_t tres = stream_resource(reinterpret_cast<const uint8_t *>(A->clauses + (size_t)qn * A->clause_stride), cols * 4u);
#pragma unroll
        for (uint32_t u = 0; u < XPT; ++u)  // (the whole offset in the vector operand: the scalar offset of a buffer load is not checked)
            tr[u] = __builtin_amdgcn_raw_buffer_load_b32(tres, (tid + 512u * u) * 4u, 0, 0);
    };

    for (uint32_t q = 0; q < match_args()->n_q; ++q) {
        uint32_t f0, n;
        first_partition(f0, n);
        request_table(q);
        request_first(q, f0, n);
        // hand-over of the table: every wave is through with the previous query's
        if (q != 0u) __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < XPT; ++u) L.table[tid + 512u * u] = tr[u];
        __syncthreads();
        uint32_t must, must_not, should, min_should;
        {
            const uint32_t *const pw = reinterpret_cast<const uint32_t *>(match_args()->preds + q);
            must = scalar_load(pw + 0);
            must_not = scalar_load(pw + 1);
            should = scalar_load(pw + 2);
            min_should = scalar_load(pw + 3);
        }
        uint32_t cnt = 0u;  // matching rows of the wave (wave-uniform, an SGPR)

        for (uint32_t part = part0; part < stream_args()->n_parts; part += (blockDim.x >> 6) * gridDim.x) {
            if (part != part0) {  // more partitions than waves (not the case for engines built by tkspmv_create)
                TKSPMV_PARTITION_RANGE(*stream_args(), part, f0, n);
                f0 = __builtin_amdgcn_readfirstlane(f0);
                n = __builtin_amdgcn_readfirstlane(n);
                request_first(q, f0, n);
            }
            uint32_t carry = 0u;  // (a partition starts on a row boundary)
            // The ring's words in use are [dlo, dlo + dn), dn <= MATCH_RING, none beyond the word of the last expanded packet's last row.
            uint32_t dlo = 0u, dn = 0u;
            bool wrote = false;  // the partition has written a word (its first one may be shared with the partition in front)
            // Words [a, b) of the ring go to the mask and the ring is cleared: lane l takes word a + l (b - a <= MATCH_RING = 64). Zero
            // words are not written (the mask is zero already). last: the partition's closing call, whose highest word may be
            // shared with the partition behind.
            auto flush = [&](uint32_t a, uint32_t b, bool last) __attribute__((always_inline)) {
                const MatchArgs A = match_args();
                uint32_t *const out_q = A->out + (size_t)q * A->out_stride;
                const uint32_t words = A->mask_words;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint32_t w = a + lane;
                uint32_t v = 0u;
                if (lane < b - a) {
                    v = ring[w & (MATCH_RING - 1u)];
                    ring[w & (MATCH_RING - 1u)] = 0u;
                }
                const uint64_t nz = __ballot(v != 0u);
                if (nz != 0ull) {
                    const uint32_t lowest = (uint32_t)__builtin_ctzll(nz), highest = 63u - (uint32_t)__builtin_clzll(nz);
                    const bool shared = (!wrote && lane == lowest) || (last && lane == highest);
                    if (v != 0u && w < words) {
                        if (shared) (void)__hip_atomic_fetch_or(out_q + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        else out_q[w] = v;
                    }
                    wrote = true;
                }
            };
            // NBUF - 1 packets in flight behind the one being reduced; the buffers rotate by NAME (the loop is unrolled by NBUF).
            for (uint32_t i0 = 0; i0 < n; i0 += NBUF) {
#pragma unroll
                for (int u = 0; u < NBUF; ++u) {
                    const uint32_t i = i0 + (uint32_t)u;
                    if (i >= n) break;
                    const ColPkt<C> &cur = buf[u];
                    {
                        // Unconditional (offset clamped to the last packet): a fixed number of younger loads lets the compiler wait
                        // with a counted vmcnt instead of vmcnt(0).
                        load_cols_buf<C, VT>(rsrc, req_off, coff, buf[(u + NBUF - 1) % NBUF]);
                        if (i + (uint32_t)NBUF < n) req_off += P.packet_bytes;
                    }
                    const MatchWords<C> W = or_packet<C, QM>(cur, carry, tbase);
                    // The lane's union: a superset of every finished row's word in this lane. must and should can only gain from
                    // more bits, so a lane whose union fails them ends no matching row.
                    uint32_t U = W.S;
#pragma unroll
                    for (int j = 1; j < C; ++j) U |= W.s[j];
                    if (__any((U & must) == must && (uint32_t)__popc(U & should) >= min_should)) {
                        const MatchArgs A = match_args();
                        uint32_t rw[C];  // the row word at every row end (expand()'s selection)
                        rw[0] = W.S;     // if entry 0 ends a row it is the lane's first row end
                        uint32_t o = W.m[0];
#pragma unroll
                        for (int j = 1; j < C; ++j) {
                            rw[j] = (W.s[j] & o) | (W.S & ~o);  // an earlier end in the lane => s_j
                            o |= W.m[j];
                        }
                        RowSums<C> S{};  // (the flag word is all mask_rows and valid() look at)
                        S.fl = W.fl;
                        const uint32_t rb = scalar_load(stream_args()->pkt_row + f0 + i);  // first row of the packet: this path only
                        if (FILT) {
                            const FilterParams F{A->mask + (size_t)q * A->mask_stride, A->mask_words};
                            mask_rows<C>(S, rb, mask_pair(F, rb), F);
                        }
                        uint32_t pass = 0u;  // bit j: the lane's entry j ends a matching row
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const bool ok = S.valid(j) && (rw[j] & must) == must && (rw[j] & must_not) == 0u && (uint32_t)__popc(rw[j] & should) >= min_should;
                            pass |= ok ? 1u << j : 0u;
                        }
                        if (__any(pass != 0u)) {
                            // Row ends in lower lanes, in the packet, and the packet's matches: sums over the lanes of numbers of at most
                            // C, taken bit by bit -- log2(C) + 1 ballots each where one per entry would take C.
                            const uint32_t ends = (uint32_t)__popc(W.fl & ((1u << C) - 1u)), hits = (uint32_t)__popc(pass);
                            uint32_t below = 0u, n_ends = 0u, total = 0u;
#pragma unroll
                            for (int b = 0; (1 << b) <= C; ++b) {
                                const uint64_t eb = __ballot(((ends >> b) & 1u) != 0u);
                                below += __builtin_amdgcn_mbcnt_hi((uint32_t)(eb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)eb, 0u)) << b;
                                n_ends += (uint32_t)__popcll(eb) << b;
                                total += (uint32_t)__popcll(__ballot(((hits >> b) & 1u) != 0u)) << b;
                            }
                            cnt += total;
                            // The packet's rows are [rb, rb + n_ends): every word in front of rb's is complete.
                            const uint32_t w0 = rb >> 5, we = (rb + n_ends - 1u) >> 5;
                            if (dn == 0u) {
                                dlo = w0;
                            } else if (we - dlo >= MATCH_RING) {  // the ring cannot take this packet's words as well
                                flush(dlo, dlo + dn < w0 ? dlo + dn : w0, false);  // (what stays in use is word w0 alone)
                                dlo = w0;
                            }
                            dn = we - dlo + 1u;
                            // The lane's row ends are the consecutive rows r0, r0 + 1, ...: their bits, a field of C at bit r0 & 31 of a
                            // 64-bit word, reach at most two mask words -- one LDS atomic each.
                            const uint32_t r0 = rb + below;
                            uint32_t t = 0u, field = 0u;  // bit t of field: row r0 + t matches
#pragma unroll
                            for (int j = 0; j < C; ++j) {
                                field |= ((pass >> j) & 1u) << t;
                                t += (W.fl >> j) & 1u;
                            }
                            const unsigned long long bits = (unsigned long long)field << (r0 & 31u);
                            const uint32_t lo_bits = (uint32_t)bits, hi_bits = (uint32_t)(bits >> 32), aw = r0 >> 5;
                            if (lo_bits != 0u) (void)__hip_atomic_fetch_or(&ring[aw & (MATCH_RING - 1u)], lo_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (hi_bits != 0u) (void)__hip_atomic_fetch_or(&ring[(aw + 1u) & (MATCH_RING - 1u)], hi_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            }
            if (dn != 0u) flush(dlo, dlo + dn, true);
        }
        // ONE atomic per wave and query for the count.
        if (cnt != 0u) {
            uint32_t *const counts = match_args()->counts;
            if (counts != nullptr && __builtin_amdgcn_inverse_ballot_w64(1ull)) (void)__hip_atomic_fetch_add(counts + q, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace tkspmv

