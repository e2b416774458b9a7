// kernels/facet_kernel.hpp -- facet_kernel: matches and best match per label for thresholded queries (tkspmv_enqueue_facets).
// Part of engine.hip (one translation unit: included there behind the other kernel headers; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"
#include "batch_kernel.hpp"  // TKSPMV_CLOCK_STRIDE
#include "range_kernel.hpp"

namespace tkspmv {

// range_kernel's loop with another sink. Everything up to "a row passes" is range_kernel's: the trigger test, expand, mask_rows,
// row_score >= tau, the timetable, the counted waits, the hand-over of x between the queries of a launch, the stream copies. What
// differs is where a match goes: not into a list of (row, score) pairs in global memory but into the bin of its label
// -- a count, and the maximum of the 64-bit result-order key (order key of the score << 32 | global row), which names the bin's
// first match in the result order whatever order the matches arrive in. Matches still pass through the wave's private list in LDS:
// the list batches the gathers labels[row] into the flush, outside the streaming loop.
// Two regimes of deposit, wave-uniform per launch (a scalar branch on lds_bins):
//   lds_bins != 0 (n_bins <= FacetGeom<XCOLS>::BINS): a workgroup-private histogram in LDS, LDS atomics (add, 64-bit max). Inside the
//     hand-over -- behind the barrier that says every wave is through with the query, in front of the one that releases the next x --
//     the 512 threads sweep the non-zero bins to global memory (atomicAdd / atomicMax) and clear them: no barrier more than range_kernel
//     has per query, and one behind the last query.
//   lds_bins == 0: the flush goes with global atomics straight at counts / best (many bins: little contention).
// Every write is an LDS atomic or a global atomic from vector lanes. counts / best / totals are zeroed in front of the launch.
// Scalar registers: the sink adds a dozen wave-uniform values (pointers, bin count, regime) to a loop that fills the register file
// already, so the kernel is written to keep few of them alive across the packet loop, and spills none:
//   - what only the rare paths need (the hand-over, a flush, a packet that triggers, a further partition) is read from the kernel's
//     argument segment where it is needed -- scalar loads that hit the constant cache -- instead of once, up front (facet_args /
//     stream_args: the pointer goes through an empty asm, so the compiler cannot move the loads back out of those paths);
//   - x is requested through a buffer resource of cols words, which returns 0 beyond them: no compare per word;
//   - whether a flush is due is decided from the NUMBER of rows that pass; which lanes and which list slots is worked out behind
//     the flush, and kept as bits of a vector register, not as a lane mask in two scalar registers per entry.
struct FacetParams {
    const uint8_t *replicas[16];  // the copies of the packet stream (cache-defeat mode); [0] alone otherwise
    uint32_t n_replicas;
    uint32_t q0;                  // number of this launch's first query within the call (picks the stream copies)
    uint32_t n_q;
    const float *xs;              // query i of the launch: xs + i * cols
    const float *thresholds;      // [n_q]
    const uint32_t *mask;         // FILT: query i's allow-mask at mask + i * mask_stride words
    uint32_t mask_stride, mask_words;
    const uint32_t *labels;       // [rows] label of each local row; >= n_bins: the row belongs to no bin
    uint32_t n_bins;
    uint32_t lds_bins;            // != 0: the LDS regime (n_bins <= the tier's capacity, checked by the kernel too)
    uint32_t *counts;             // [n_q][n_bins] matches per bin
    unsigned long long *best;     // [n_q][n_bins] maximum of (order key << 32 | global row) per bin, or NULL
    uint32_t *totals;             // [n_q] all matches, or NULL
    uint32_t first_row;
    uint32_t period;              // the timetable (RangeParams::period)
    uint32_t args_tag;            // FACET_ARGS_TAG: the kernel finds it where it expects R in its argument segment, or traps
};
constexpr uint32_t FACET_ARGS_TAG = 0xFACE7A65u;

// Bins of the workgroup-private histogram, 12 bytes each. A CU has 160 KiB of LDS and the kernel keeps two workgroups on it: 80 KiB
// each. x and the lists take 4 + 16 = 20 KiB at 1024 columns, 16 + 8 = 24 KiB at 4096, 64 + 8 = 72 KiB at 16384: 4096 bins (48 KiB)
// fit the first two, 512 bins (6 KiB) the last.
template <int XCOLS>
struct FacetGeom {
    static constexpr uint32_t BINS = XCOLS <= 4096 ? 4096u : 512u;
};
constexpr uint32_t facet_lds_bins(int xcols) { return xcols <= 4096 ? FacetGeom<1024>::BINS : FacetGeom<16384>::BINS; }

template <int XCOLS>
struct FacetLds {
    float x[XCOLS];                          // at LDS offset 0: (column word & 0xFFC) | xbase is the address of x[col]
    uint2 cand[ListGeom<XCOLS>::CAND_CAP];   // private lists of the 8 waves {score bits, local row}
    unsigned long long hbest[FacetGeom<XCOLS>::BINS];
    uint32_t hcount[FacetGeom<XCOLS>::BINS];
};
static_assert(sizeof(FacetLds<1024>) <= 80u * 1024u && sizeof(FacetLds<4096>) <= 80u * 1024u && sizeof(FacetLds<16384>) <= 80u * 1024u,
              "two workgroups of facet_kernel per CU");

template <int C, int XCOLS, int QM, bool FILT, int NBUF>
__global__ void __launch_bounds__(512, 4) facet_kernel(const StreamParams P, const FacetParams R) {
    static_assert((QM == QM_F32 || QM == QM_F32C12) && (C == 4 || C == 8), "facet_kernel: fp32 packet streams of 4 or 8 entries per lane");
    constexpr int VT = value_type_of(QM);
    constexpr bool BUF = C == 4;  // buffer loads (load_packet_buf) where they exist
    constexpr uint32_t WAVE_CAP = ListGeom<XCOLS>::WAVE_CAP;
    constexpr uint32_t XPT = (uint32_t)XCOLS / 512u;  // words of x per thread
    static_assert(XCOLS % 512 == 0, "x is staged by 512 threads");
    __shared__ FacetLds<XCOLS> L;
    // (reduce_packet forms LDS addresses of x as (word & 0xFFC) | base: x must sit on a 4 KiB boundary -- this object is the
    //  kernel's ONLY __shared__ block, so it starts at LDS address 0, and x is its first member)
    static_assert(offsetof(FacetLds<XCOLS>, x) == 0, "x must be the first member of the kernel's LDS block");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bid = blockIdx.x, n_wg = gridDim.x;
    const uint32_t total_waves = (blockDim.x >> 6) * n_wg;
    const uint32_t part0 = wave * n_wg + bid;
    const uint32_t xbase = lds_addr_of(L.x);
    uint2 *wcand = L.cand + wave * WAVE_CAP;
    const uint32_t wave_entry_fp = (uint32_t)__builtin_amdgcn_s_memrealtime() << 8;
    // P and R as they lie in the kernel's argument segment, for the rare paths: a field read through these is loaded where it is
    // used. The rule relied on is the AMDGPU HSA code-object ABI's (LLVM AMDGPUUsage, "Kernel Argument Processing" / the .args
    // metadata): the explicit arguments lie in declaration order, each at the next offset aligned for its type, a struct passed by
    // value in place -- so P at 0 and R at sizeof(StreamParams). The hot fields (P.packet_bytes, R.period, the first partition's
    // table) are read the ordinary way; both views are of the same bytes. Guards: the static_assert on padding, and args_tag -- every
    // wave compares the tag and two fields of either view at entry and traps on a mismatch, so an argument list or a lowering that
    // breaks the rule fails every launch (tests/test_gpu_facets.py) instead of reading other bytes.
    typedef const char __attribute__((address_space(4))) *ArgBytes;
    typedef const FacetParams __attribute__((address_space(4))) *FacetArgs;
    typedef const StreamParams __attribute__((address_space(4))) *StreamArgs;
    static_assert(sizeof(StreamParams) % alignof(FacetParams) == 0, "R follows P without padding");
    auto arg_segment = [&]() __attribute__((always_inline)) {
        ArgBytes a = (ArgBytes)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(a));
        return a;
    };
    auto stream_args = [&]() __attribute__((always_inline)) { return (StreamArgs)arg_segment(); };
    auto facet_args = [&]() __attribute__((always_inline)) { return (FacetArgs)(arg_segment() + sizeof(StreamParams)); };
    if (facet_args()->args_tag != FACET_ARGS_TAG || facet_args()->n_q != R.n_q || stream_args()->n_parts != P.n_parts) __builtin_trap();
    // The regime (launch parameters: the same for every wave).
    auto lds_regime = [&]() __attribute__((always_inline)) {
        const FacetArgs A = facet_args();
        return A->lds_bins != 0u && A->n_bins <= FacetGeom<XCOLS>::BINS;
    };

    uint32_t p0 = 0, np = 0;  // the wave's first partition (the same for every query)
    if (part0 < P.n_parts) TKSPMV_PARTITION_RANGE(P, part0, p0, np);
    p0 = __builtin_amdgcn_readfirstlane(p0);
    np = __builtin_amdgcn_readfirstlane(np);
    const uint32_t tpkt_fp = (R.period != 0u && np != 0u) ? (uint32_t)((float)R.period / (float)np) : 0u;  // a packet's slot on the timetable
    uint32_t sched_fp = wave_entry_fp;  // when the packet being reduced is due (ticks << 8, low 32 bits)

    Pkt<C, VT> buf[NBUF];
    LaneOffsets lo{0u, 0u};
    if constexpr (BUF) lo = lane_offsets<C, VT>(lane);
    const uint8_t *pk = R.replicas[0];
    __amdgpu_buffer_rsrc_t rsrc = stream_resource(pk, 0u);
    uint32_t req_off = 0u;
    // The first NBUF - 1 packets of partition [f0, f0 + n) in the stream copy of query qn (clamped to the last packet).
    auto request_first = [&](uint32_t qn, uint32_t f0, uint32_t n) __attribute__((always_inline)) {
        const FacetArgs A = facet_args();
        pk = A->replicas[(A->q0 + qn) % A->n_replicas] + (size_t)f0 * P.packet_bytes;
        if constexpr (BUF) rsrc = stream_resource(pk, n * P.packet_bytes);
#pragma unroll
        for (int u = 0; u < NBUF - 1; ++u) {
            const uint32_t iu = ((uint32_t)u < n) ? (uint32_t)u : (n > 0u ? n - 1u : 0u);
            // (a resource of 0 bytes returns 0 and touches nothing: no branch around the loads of a wave without a partition)
            if constexpr (BUF) load_packet_buf<C, VT>(rsrc, iu * P.packet_bytes, lo, buf[u]);
            else if (n > 0u) load_packet<C, VT>(pk + (size_t)iu * P.packet_bytes, lane, buf[u]);
        }
        req_off = (n > (uint32_t)(NBUF - 1) ? (uint32_t)(NBUF - 1) : (n > 0u ? n - 1u : 0u)) * P.packet_bytes;  // the next request's packet
    };
    // x of query qn, XPT words per thread (the loads are issued back to back, ahead of the packets)
    float xr[XPT];
    auto request_x = [&](uint32_t qn) __attribute__((always_inline)) {
        // (a buffer resource of cols words: a word beyond it reads as 0 without a compare per word, whose lane masks -- XPT of them,
        //  32 at 16384 columns -- would otherwise sit in scalar registers until the loads have been issued)
        const uint32_t cols = stream_args()->cols;
        const __amdgpu_buffer_rsrc_t xres = stream_resource(reinterpret_cast<const uint8_t *>(facet_args()->xs + (size_t)qn * cols), cols * 4u);
#pragma unroll
        for (uint32_t t = 0; t < XPT; ++t)  // (the whole offset in the vector operand: the scalar offset of a buffer load is not checked)
            xr[t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (tid + 512u * t) * 4u, 0, 0));
    };
    // The workgroup's histogram of query qd to global memory, non-zero bins only, each cleared by the thread that swept it.
    auto sweep = [&](uint32_t qd) __attribute__((always_inline)) {
        const FacetArgs A = facet_args();
        const uint32_t n_bins = A->n_bins;
        const bool want_best = A->best != nullptr;
        uint32_t *const cq = A->counts + (size_t)qd * n_bins;
        unsigned long long *const bq = A->best + (size_t)qd * n_bins;
        for (uint32_t b = tid; b < n_bins; b += 512u) {
            const uint32_t c = L.hcount[b];
            if (c != 0u) {
                (void)__hip_atomic_fetch_add(cq + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                L.hcount[b] = 0u;
                if (want_best) {
                    (void)__hip_atomic_fetch_max(bq + b, L.hbest[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    L.hbest[b] = 0ull;
                }
            }
        }
    };

    for (uint32_t q = 0; q < facet_args()->n_q; ++q) {
        // The query's x and the first packets of its first partition are requested before the hand-over's barriers (the buffers are
        // free: the previous query's last packet has been reduced), so they travel while the slower waves of the workgroup finish.
        request_x(q);
        request_first(q, p0, np);
        // hand-over: every wave is through with the previous query's x -- and with its deposits
        if (q != 0u) __syncthreads();
        if (lds_regime()) {
            if (q != 0u) {
                sweep(q - 1u);
            } else {
                for (uint32_t b = tid, n_bins = facet_args()->n_bins; b < n_bins; b += 512u) {
                    L.hcount[b] = 0u;
                    L.hbest[b] = 0ull;
                }
            }
        }
#pragma unroll
        for (uint32_t t = 0; t < XPT; ++t) L.x[tid + 512u * t] = xr[t];
        __syncthreads();
        const float tau = __uint_as_float(scalar_load(reinterpret_cast<const uint32_t *>(facet_args()->thresholds) + q));
        uint32_t wcnt = 0u;  // length of the wave's list (wave-uniform, an SGPR)
        struct Sink {
            const uint32_t *labels;
            uint32_t *count_q;
            unsigned long long *best_q;
            uint32_t *total_q;
            uint32_t n_bins, first_row;
            bool in_lds;
        };
        auto sink_of = [&]() __attribute__((always_inline)) {
            const FacetArgs A = facet_args();
            Sink K;
            K.labels = A->labels;
            K.n_bins = A->n_bins;
            K.first_row = A->first_row;
            K.in_lds = lds_regime();
            K.count_q = A->counts + (size_t)q * K.n_bins;
            K.best_q = A->best ? A->best + (size_t)q * K.n_bins : nullptr;
            K.total_q = A->totals ? A->totals + q : nullptr;
            return K;
        };
        // One match into the bin of its label (a lane each; a label beyond the bins: nowhere).
        auto deposit = [&](const Sink &K, uint32_t lab, uint32_t row, uint32_t bits) __attribute__((always_inline)) {
            const bool want_best = K.best_q != nullptr;
            uint32_t *const count_q = K.count_q;
            unsigned long long *const best_q = K.best_q;
            if (lab < K.n_bins) {
                const unsigned long long key = ((unsigned long long)order_key(__uint_as_float(bits)) << 32) | (unsigned long long)(row + K.first_row);
                if (K.in_lds) {
                    (void)__hip_atomic_fetch_add(&L.hcount[lab], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (want_best) (void)__hip_atomic_fetch_max(&L.hbest[lab], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    (void)__hip_atomic_fetch_add(count_q + lab, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (want_best) (void)__hip_atomic_fetch_max(best_q + lab, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        };
        // Flush: ONE atomic on the query's total (lane 0), the labels of the list's rows gathered back to back, then the deposits.
        auto flush = [&]() __attribute__((always_inline)) {
            const Sink K = sink_of();
            if (K.total_q != nullptr && lane == 0) (void)__hip_atomic_fetch_add(K.total_q, wcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint2 e[WAVE_CAP / 64u];
            uint32_t lab[WAVE_CAP / 64u];
#pragma unroll
            for (uint32_t u = 0; u < WAVE_CAP / 64u; ++u) {
                const uint32_t i = lane + 64u * u;
                e[u] = make_uint2(0u, 0u);
                lab[u] = 0xFFFFFFFFu;
                if (i < wcnt) {
                    e[u] = wcand[i];
                    lab[u] = K.labels[e[u].y];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < WAVE_CAP / 64u; ++u) {
                if (lane + 64u * u < wcnt) deposit(K, lab[u], e[u].y, e[u].x);
            }
            wcnt = 0u;
        };

        uint32_t f0 = p0, n = np;
        for (uint32_t part = part0; part < stream_args()->n_parts; part += total_waves) {
            if (part != part0) {  // more partitions than waves (not the case for engines built by tkspmv_create)
                TKSPMV_PARTITION_RANGE(*stream_args(), part, f0, n);
                f0 = __builtin_amdgcn_readfirstlane(f0);
                n = __builtin_amdgcn_readfirstlane(n);
                request_first(q, f0, n);
            }
            float carry = 0.0f;  // (a partition starts on a row boundary)
            if (tpkt_fp != 0u && (n & (uint32_t)(TKSPMV_CLOCK_STRIDE - 1)) != 0u)  // (the partition's last look covers fewer packets than it books)
                sched_fp -= tpkt_fp * ((uint32_t)TKSPMV_CLOCK_STRIDE - (n & (uint32_t)(TKSPMV_CLOCK_STRIDE - 1)));
            // NBUF - 1 packets in flight behind the one being reduced; the buffers rotate by NAME (the loop is unrolled by NBUF).
            for (uint32_t i0 = 0; i0 < n; i0 += NBUF) {
#pragma unroll
                for (int u = 0; u < NBUF; ++u) {
                    const uint32_t i = i0 + (uint32_t)u;
                    if (i >= n) break;
                    const Pkt<C, VT> &cur = buf[u];
                    {
                        // Unconditional (offset clamped to the last packet): a fixed number of younger loads lets the compiler wait
                        // with a counted vmcnt instead of vmcnt(0).
                        if constexpr (BUF) load_packet_buf<C, VT>(rsrc, req_off, lo, buf[(u + NBUF - 1) % NBUF]);
                        else load_packet<C, VT>(pk + req_off, lane, buf[(u + NBUF - 1) % NBUF]);
                        if (i + (uint32_t)NBUF < n) req_off += P.packet_bytes;
                    }
                    // (the clock is asked for here and looked at behind the packet's arithmetic)
                    const bool look = tpkt_fp != 0u && (i & (uint32_t)(TKSPMV_CLOCK_STRIDE - 1)) == 0u;
                    uint32_t clk_now = 0u;
                    if (look) clk_now = (uint32_t)__builtin_amdgcn_s_memrealtime();
                    const Reduced<C> Rd = reduce_packet<C, QM>(cur, carry, xbase, 0u);
                    const float trig = trigger_of<C, false>(Rd);
                    if (look) {
                        sched_fp += tpkt_fp * (uint32_t)TKSPMV_CLOCK_STRIDE;
                        const int32_t ahead = (int32_t)(sched_fp - (clk_now << 8));  // ticks << 8
                        // (steps of 512 cycles, never longer than one period per look: range_kernel.hpp)
                        int32_t cap = (int32_t)R.period;
                        asm volatile("" : "+s"(cap));  // (2 * cap and -cap are formed here, not kept in registers of their own)
#pragma unroll 1
                        for (int32_t z = ahead < cap ? ahead : cap; z > (int32_t)(11u << 8); z -= (int32_t)(21u << 8)) __builtin_amdgcn_s_sleep(8);
                        if (ahead > 2 * cap) sched_fp = clk_now << 8;
                        if (ahead < -cap) sched_fp -= (uint32_t)(ahead + cap);
                    }
                    if (__any(trig >= tau)) {
                        // (the trigger bounds every finished row of its lane from above: packet_math.hpp)
                        RowSums<C> S = expand<C, false>(Rd, packet_flags<C, QM>(cur));
                        const uint32_t rb = scalar_load(stream_args()->pkt_row + f0 + i);  // first row of the packet: the rare path only
                        if (FILT) {
                            const FacetArgs A = facet_args();
                            const FilterParams F{A->mask + (size_t)q * A->mask_stride, A->mask_words};
                            mask_rows<C>(S, rb, mask_pair(F, rb), F);
                        }
                        // How many rows pass is all the decision to flush needs; which lanes and which slots is worked out behind
                        // the flush (fl goes through an empty asm there), so that no lane mask stays live across it.
                        uint32_t total = 0u;
#pragma unroll
                        for (int j = 0; j < C; ++j) total += (uint32_t)__popcll(__ballot(S.valid(j) && row_score<C, QM>(S, j) >= tau));
                        if (total != 0u) {
                            if (wcnt + total > WAVE_CAP) flush();
                            asm volatile("" : "+v"(S.fl));
                            // (which entries of the lane pass: bits of a vector register, tested where they are used -- a bool each would
                            //  be a lane mask in two scalar registers, C of them live down to the last deposit)
                            uint32_t pbits = 0u;
                            uint32_t slot[C];
                            uint32_t at = 0u;
                            const uint32_t below = ends_below<C>(S);
#pragma unroll
                            for (int j = 0; j < C; ++j) {
                                const bool pj = S.valid(j) && row_score<C, QM>(S, j) >= tau;
                                const uint64_t pb = __ballot(pj);
                                slot[j] = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(pb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pb, 0u));
                                at += (uint32_t)__popcll(pb);
                                pbits |= pj ? 1u << j : 0u;
                            }
                            asm volatile("" : "+v"(pbits), "+v"(S.fl));
                            auto pass = [&](int j) __attribute__((always_inline)) { return ((pbits >> j) & 1u) != 0u; };
                            uint32_t r = rb + below;
                            if (total > WAVE_CAP) {
                                // more rows in one packet than the list holds (a threshold most rows pass): straight to the bins
                                const Sink K = sink_of();
                                if (K.total_q != nullptr && lane == 0) (void)__hip_atomic_fetch_add(K.total_q, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                uint32_t lab[C], rr[C];
#pragma unroll
                                for (int j = 0; j < C; ++j) {
                                    rr[j] = r;
                                    lab[j] = pass(j) ? K.labels[r] : 0xFFFFFFFFu;
                                    r += S.end(j) ? 1u : 0u;
                                }
#pragma unroll
                                for (int j = 0; j < C; ++j) {
                                    if (pass(j)) deposit(K, lab[j], rr[j], __float_as_uint(row_score<C, QM>(S, j)));
                                }
                            } else {
#pragma unroll
                                for (int j = 0; j < C; ++j) {
                                    if (pass(j)) wcand[wcnt + slot[j]] = make_uint2(__float_as_uint(row_score<C, QM>(S, j)), r);
                                    r += S.end(j) ? 1u : 0u;
                                }
                                wcnt += total;
                            }
                        }
                    }
                }
            }
        }
        if (wcnt != 0u) flush();
    }
    if (lds_regime()) {  // the last query's histogram, once every wave's deposits are in
        __syncthreads();
        sweep(facet_args()->n_q - 1u);
    }
}

// Closing launch over the count * n_bins entries of best: a non-zero entry (order key << 32 | global row) becomes the caller's record
// {row, score bits} -- the high word goes back through the inverse of order_key, the low word stays. Zero entries stay {0, 0}.
__global__ void __launch_bounds__(256) facet_close_kernel(unsigned long long *best, unsigned long long n) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long v = best[i];
        if (v != 0ull) best[i] = ((unsigned long long)__float_as_uint(key_to_float((uint32_t)(v >> 32))) << 32) | (v & 0xFFFFFFFFull);
    }
}

}  // namespace tkspmv
