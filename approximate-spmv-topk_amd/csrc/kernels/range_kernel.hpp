// kernels/range_kernel.hpp -- range_kernel: every row scoring at least a per-query threshold (tkspmv_enqueue_range).
// Part of engine.hip (one translation unit: included there behind the other kernel headers; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"
#include "batch_kernel.hpp"  // TKSPMV_CLOCK_STRIDE

namespace tkspmv {

// The streaming loop at its simplest. The threshold of a range query is the caller's and is known before the first packet, so
// there is no threshold exchange, no cold start, no deferred packet, no server wave, no published maximum, no check, no repair
// and no selection -- and no workgroup ever waits for another. Per packet: reduce, compare the lane's trigger_of() against the
// threshold, and only if some lane passes expand the row sums and append the rows that qualify to the wave's private list in
// LDS. The trigger is the maximum of a set that contains every finished row's sum (packet_math.hpp), whatever the signs of the
// products, so it can fire for nothing but never miss a row; the comparison that decides is row_score >= threshold on the fp32
// value the caller receives. A masked row end (FILT) is marked like the placeholder of an empty row right behind expand(): fewer
// rows keep the trigger an upper bound.
// One launch serves n_q queries: a workgroup walks its partitions once per query, then hands x over (request the next x and the
// next query's first packets, barrier, stage, barrier) and takes the next one. Query i reads stream copy (q0 + i) % n_replicas.
struct RangeParams {
    const uint8_t *replicas[16];  // the copies of the packet stream (cache-defeat mode); [0] alone otherwise
    uint32_t n_replicas;
    uint32_t q0;                  // number of this launch's first query within the call (picks the stream copies)
    uint32_t n_q;
    const float *xs;              // query i of the launch: xs + i * cols
    const float *thresholds;      // [n_q]
    const uint32_t *mask;         // FILT: query i's allow-mask at mask + i * mask_stride words
    uint32_t mask_stride, mask_words;
    uint32_t *counts;             // [n_q] matches found (zeroed in front of the launch), also beyond capacity
    uint32_t *idx;                // [n_q][capacity] row ids (+ first_row), no particular order
    float *val;                   // [n_q][capacity] their scores
    uint32_t capacity;
    uint32_t first_row;
    // The timetable (BatchParams::pace_period, ReadProbeParams::period): ticks << 8 per query, 0 = unpaced. Packet j of query q is due
    // at (the wave's entry) + (q x packets + j) x period / packets; a wave sleeps off its lead every TKSPMV_CLOCK_STRIDE packets,
    // behind the packet's arithmetic. A wave that is behind never pauses.
    uint32_t period;
};

template <int XCOLS>
struct RangeLds {
    float x[XCOLS];                          // at LDS offset 0: (column word & 0xFFC) | xbase is the address of x[col]
    uint2 cand[ListGeom<XCOLS>::CAND_CAP];   // private lists of the 8 waves {score bits, local row}
};

template <int C, int XCOLS, int QM, bool FILT, int NBUF>
__global__ void __launch_bounds__(512, 4) range_kernel(const StreamParams P, const RangeParams R) {
    static_assert((QM == QM_F32 || QM == QM_F32C12) && (C == 4 || C == 8), "range_kernel: fp32 packet streams of 4 or 8 entries per lane");
    constexpr int VT = value_type_of(QM);
    constexpr bool BUF = C == 4;  // buffer loads (load_packet_buf) where they exist
    constexpr uint32_t WAVE_CAP = ListGeom<XCOLS>::WAVE_CAP;
    constexpr uint32_t XPT = (uint32_t)XCOLS / 512u;  // words of x per thread
    static_assert(XCOLS % 512 == 0, "x is staged by 512 threads");
    __shared__ RangeLds<XCOLS> L;
    // (reduce_packet forms LDS addresses of x as (word & 0xFFC) | base: x must sit on a 4 KiB boundary -- this object is the
    //  kernel's ONLY __shared__ block, so it starts at LDS address 0, and x is its first member)
    static_assert(offsetof(RangeLds<XCOLS>, x) == 0, "x must be the first member of the kernel's LDS block");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bid = blockIdx.x, n_wg = gridDim.x;
    const uint32_t total_waves = (blockDim.x >> 6) * n_wg;
    const uint32_t part0 = wave * n_wg + bid;
    const uint32_t xbase = lds_addr_of(L.x);
    uint2 *wcand = L.cand + wave * WAVE_CAP;
    const uint32_t wave_entry_fp = (uint32_t)__builtin_amdgcn_s_memrealtime() << 8;

    uint32_t p0 = 0, np = 0;  // the wave's first partition (the same for every query)
    if (part0 < P.n_parts) TKSPMV_PARTITION_RANGE(P, part0, p0, np);
    // (wave-uniform by construction; said so, or a table read with vector loads makes every packet offset a vector value and each
    //  buffer load a loop over its lanes)
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
        pk = R.replicas[(R.q0 + qn) % R.n_replicas] + (size_t)f0 * P.packet_bytes;
        if constexpr (BUF) rsrc = stream_resource(pk, n * P.packet_bytes);
#pragma unroll
        for (int u = 0; u < NBUF - 1; ++u) {
            const uint32_t iu = ((uint32_t)u < n) ? (uint32_t)u : (n > 0u ? n - 1u : 0u);
            // (buffer loads of a wave without a partition: a resource of 0 bytes returns 0 and touches nothing -- no branch around
            //  the loads, so the wait for x in front of them stays a counted one)
            if constexpr (BUF) load_packet_buf<C, VT>(rsrc, iu * P.packet_bytes, lo, buf[u]);
            else if (n > 0u) load_packet<C, VT>(pk + (size_t)iu * P.packet_bytes, lane, buf[u]);
        }
        req_off = (n > (uint32_t)(NBUF - 1) ? (uint32_t)(NBUF - 1) : (n > 0u ? n - 1u : 0u)) * P.packet_bytes;  // the next request's packet
    };
    // x of query qn, XPT words per thread (clamped addresses, masked values: the loads are issued back to back, ahead of the packets)
    float xr[XPT];
    auto request_x = [&](uint32_t qn) __attribute__((always_inline)) {
        const float *x = R.xs + (size_t)qn * P.cols;
#pragma unroll
        for (uint32_t t = 0; t < XPT; ++t) {
            const uint32_t i = tid + 512u * t;
            const float xw = x[i < P.cols ? i : 0u];
            xr[t] = i < P.cols ? xw : 0.0f;
        }
    };

    for (uint32_t q = 0; q < R.n_q; ++q) {
        // The query's x and the first packets of its first partition are requested before the hand-over's barriers (the buffers are
        // free: the previous query's last packet has been reduced), so they travel while the slower waves of the workgroup finish.
        request_x(q);
        request_first(q, p0, np);
        // hand-over of x: every wave is through with the previous query's x
        if (q != 0u) __syncthreads();
#pragma unroll
        for (uint32_t t = 0; t < XPT; ++t) L.x[tid + 512u * t] = xr[t];
        __syncthreads();
        const float tau = __uint_as_float(scalar_load(reinterpret_cast<const uint32_t *>(R.thresholds) + q));
        const FilterParams F{FILT ? R.mask + (size_t)q * R.mask_stride : nullptr, R.mask_words};
        uint32_t *const count_q = R.counts + q;
        uint32_t *const idx_q = R.idx + (size_t)q * R.capacity;
        float *const val_q = R.val + (size_t)q * R.capacity;
        uint32_t wcnt = 0u;  // length of the wave's list (wave-uniform, an SGPR)
        // Flush: ONE atomic on the query's counter (lane 0), then coalesced plain stores. Nothing reads them inside the launch.
        auto flush = [&]() __attribute__((always_inline)) {
            uint32_t gbase = 0u;
            if (lane == 0) gbase = atomicAdd(count_q, wcnt);
            gbase = __builtin_amdgcn_readfirstlane(gbase);
#pragma unroll
            for (uint32_t u = 0; u < WAVE_CAP / 64u; ++u) {
                const uint32_t i = lane + 64u * u;
                if (i < wcnt && gbase + i < R.capacity) {
                    const uint2 e = wcand[i];
                    idx_q[gbase + i] = e.y + R.first_row;
                    val_q[gbase + i] = __uint_as_float(e.x);
                }
            }
            wcnt = 0u;
        };

        uint32_t f0 = p0, n = np;
        for (uint32_t part = part0; part < P.n_parts; part += total_waves) {
            if (part != part0) {  // more partitions than waves (not the case for engines built by tkspmv_create)
                TKSPMV_PARTITION_RANGE(P, part, f0, n);
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
                        // (steps of 512 cycles, never longer than one period per look: whatever says the wave is further ahead -- a
                        //  clock that wrapped, a period of another matrix -- costs a bounded pause; a debt stops growing at one query)
                        const int32_t cap = (int32_t)R.period;
#pragma unroll 1
                        for (int32_t z = ahead < cap ? ahead : cap; z > (int32_t)(11u << 8); z -= (int32_t)(21u << 8)) __builtin_amdgcn_s_sleep(8);
                        if (ahead > 2 * cap) sched_fp = clk_now << 8;
                        if (ahead < -cap) sched_fp -= (uint32_t)(ahead + cap);
                    }
                    if (__any(trig >= tau)) {
                        // (the trigger bounds every finished row of its lane from above: packet_math.hpp)
                        RowSums<C> S = expand<C, false>(Rd, packet_flags<C, QM>(cur));
                        const uint32_t rb = scalar_load(P.pkt_row + f0 + i);  // first row of the packet: the rare path only
                        if (FILT) mask_rows<C>(S, rb, mask_pair(F, rb), F);
                        bool pass[C];
                        uint32_t slot[C];
                        uint32_t total = 0u;
                        const uint32_t below = ends_below<C>(S);
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            pass[j] = S.valid(j) && row_score<C, QM>(S, j) >= tau;
                            const uint64_t pb = __ballot(pass[j]);
                            slot[j] = total + __builtin_amdgcn_mbcnt_hi((uint32_t)(pb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pb, 0u));
                            total += (uint32_t)__popcll(pb);
                        }
                        if (total != 0u) {
                            if (wcnt + total > WAVE_CAP) flush();
                            uint32_t r = rb + below;
                            if (total > WAVE_CAP) {
                                // more rows in one packet than the list holds (a threshold most rows pass): straight to the output
                                uint32_t gbase = 0u;
                                if (lane == 0) gbase = atomicAdd(count_q, total);
                                gbase = __builtin_amdgcn_readfirstlane(gbase);
#pragma unroll
                                for (int j = 0; j < C; ++j) {
                                    if (pass[j] && gbase + slot[j] < R.capacity) {
                                        idx_q[gbase + slot[j]] = r + R.first_row;
                                        val_q[gbase + slot[j]] = row_score<C, QM>(S, j);
                                    }
                                    r += S.end(j) ? 1u : 0u;
                                }
                            } else {
#pragma unroll
                                for (int j = 0; j < C; ++j) {
                                    if (pass[j]) wcand[wcnt + slot[j]] = make_uint2(__float_as_uint(row_score<C, QM>(S, j)), r);
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
}

}  // namespace tkspmv
