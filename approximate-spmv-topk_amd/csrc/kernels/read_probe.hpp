// kernels/read_probe.hpp -- measurement aid: the packet stream read and nothing else (read_probe_kernel).
// Part of engine.hip (one translation unit; device code only).
#pragma once
#include "common.hpp"
#include "packet_math.hpp"

namespace tkspmv {

// What does it cost on THIS GPU to move the matrix stream from HBM into registers, with the engine's own geometry (same
// grid, same waves, same partition of the stream among them, the same wide non-temporal loads) and no arithmetic, no
// x, no selection? bench.py reports the streaming kernels against this figure beside the 8 TB/s specification: boxes of
// one pool differ by several per cent, and the best plain copy the microarchitecture guide measured is 6.29 TB/s.
// One launch makes n_pass passes (rotating the stream copies like the batch kernel), so that no launch boundary falls
// into the timed region. Every loaded word is folded into a value that is stored once per wave (the loads cannot be
// dropped by the compiler).
struct ReadProbeParams {
    const uint8_t *replicas[8];
    uint32_t n_replicas;
    const uint32_t *part_first, *part_count;
    uint32_t n_parts, n_pass;
    uint32_t map;  // 0: the engine's partition of wave w of workgroup b (w * grid + b); 1, 2: XCD-contiguous variants (tuning runs)
    uint32_t *sink;  // [grid * waves]
    uint32_t *claim;  // map 3: [n_pass] counters, 32 words apart, zeroed: waves claim their partitions instead of owning them
    unsigned long long *t_end;  // [grid * waves] (optional) s_memrealtime when the wave has finished its last pass
    // Round 5: the probe on a timetable (batch_kernel.hpp, BatchParams::pace_period). Left alone the probe's waves ask for all they
    // can get and the memory system serves four XCDs at twice the others' rate -- on some boxes the "floor" it measures is a pass the
    // paced product beats. period != 0 (ticks << 8 per pass): a wave sleeps off what it is ahead of packet j's slot, (its start) +
    // (pass x packets + j) x period / packets, looked at every DEPTH packets. The smallest time over a handful of periods is the
    // figure bench.py reports as `read_only.paced_us`.
    uint32_t period;
};

template <int BPL>  // bytes per lane and packet: 22 (fp32 + 12-bit column words), 24 (fp32, C = 4), 48 (fp32, C = 8), 16 (FIXED20), 12 (byte / half values)
__device__ __forceinline__ uint32_t read_probe_packet(const uint8_t *__restrict__ pk, uint32_t lane) {
    uint32_t acc = 0u;
    if (BPL == 22) {  // values as they are, 12-bit column words: two lanes share three dwords (overlapping dwordx2 loads)
        const f32x4 f = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(pk + lane * 16));
        const u32x2 c = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(pk + 1024 + (lane >> 1) * 12 + (lane & 1u) * 4));
        acc ^= __float_as_uint(f.x) ^ __float_as_uint(f.y) ^ __float_as_uint(f.z) ^ __float_as_uint(f.w) ^ c.x ^ c.y;
    } else if (BPL == 24 || BPL == 48) {
#pragma unroll
        for (int q = 0; q < BPL / 24; ++q) {
            const f32x4 f = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(pk + q * 1024 + lane * 16));
            const u32x2 c = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(pk + (BPL / 24) * 1024 + q * 512 + lane * 8));
            acc ^= __float_as_uint(f.x) ^ __float_as_uint(f.y) ^ __float_as_uint(f.z) ^ __float_as_uint(f.w) ^ c.x ^ c.y;
        }
    } else if (BPL == 20) {  // FIXED26: 16 + 4 bytes per lane
        const f32x4 f = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(pk + lane * 16));
        const uint32_t e = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(pk + 1024 + lane * 4));
        acc ^= __float_as_uint(f.x) ^ __float_as_uint(f.y) ^ __float_as_uint(f.z) ^ __float_as_uint(f.w) ^ e;
    } else if (BPL == 16) {
        const f32x4 f = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(pk + lane * 16));
        acc ^= __float_as_uint(f.x) ^ __float_as_uint(f.y) ^ __float_as_uint(f.z) ^ __float_as_uint(f.w);
    } else {
        const uint32_t v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(pk + lane * 4));
        const u32x2 c = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(pk + 256 + lane * 8));
        acc ^= v ^ c.x ^ c.y;
    }
    return acc;
}

// DEPTH: packets in flight per wave; WORK: dependent vector instructions spent per packet on what was loaded (tuning
// runs, TKSPMV_READ_PROBE=depth,work: how the floor moves with the prefetch depth and with arithmetic in the loop)
template <int BPL, int DEPTH = 8, int WORK = 0>
__global__ void __launch_bounds__(1024) read_probe_kernel(const ReadProbeParams R) {
    constexpr uint32_t PB = (BPL == 22 && WORK == 1 ? 24 : BPL) * 64u;  // (22 with WORK 1: 1408-byte packets read out of a 1536-byte stream)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    uint32_t acc = 0u;
    uint32_t sched_fp = 0u;  // (the probe's timetable: ReadProbeParams::period)
    __shared__ float xl[WORK < 0 ? 1024 : 1];
    if (WORK < 0) {
        for (uint32_t i = threadIdx.x; i < 1024u; i += blockDim.x) xl[i] = 1.0f + (float)(i & 7u);
        __syncthreads();
    }
    if (R.map == 4u) {
        // map 4: the WORKGROUP claims sets of n_waves partitions (one atomic per set, prefetched: the next set is claimed
        // before the current one is streamed, so the counter's round trip is off the path)
        __shared__ uint32_t set_lds[2];
        const uint32_t n_sets = (R.n_parts + n_waves - 1u) / n_waves;
        for (uint32_t pass = 0; pass < R.n_pass; ++pass) {
            const uint8_t *base = R.replicas[pass % R.n_replicas];
            if (threadIdx.x == 0) set_lds[0] = atomicAdd(&R.claim[32u * pass], 1u);
            __syncthreads();
            for (uint32_t it = 0;; ++it) {
                const uint32_t sset = set_lds[it & 1u];
                if (sset >= n_sets) break;
                uint32_t nxt = 0u;
                if (threadIdx.x == 0) nxt = atomicAdd(&R.claim[32u * pass], 1u);
                const uint32_t p = sset * n_waves + wave;
                if (p < R.n_parts) {
                    const uint32_t first = R.part_first[p], count = R.part_count[p];
                    const uint8_t *pk = base + (size_t)first * PB;
                    uint32_t i = 0;
                    for (; i + DEPTH <= count; i += DEPTH) {
#pragma unroll
                        for (int j = 0; j < DEPTH; ++j) acc ^= read_probe_packet<BPL>(pk + (size_t)(i + j) * PB, lane);
                    }
                    for (; i < count; ++i) acc ^= read_probe_packet<BPL>(pk + (size_t)i * PB, lane);
                }
                if (threadIdx.x == 0) set_lds[(it + 1u) & 1u] = nxt;
                __syncthreads();
            }
            __syncthreads();
        }
    } else
    for (uint32_t pass = 0; pass < R.n_pass; ++pass) {
        const uint8_t *base = R.replicas[pass % R.n_replicas];
        uint32_t p_first = wave * gridDim.x + blockIdx.x;
        if (R.map != 0u) {  // workgroups are dealt to the 8 XCDs round-robin: give every XCD one contiguous eighth of the stream
            const uint32_t xcd = blockIdx.x & 7u, li = blockIdx.x >> 3, per_xcd = (gridDim.x >> 3) * n_waves;
            p_first = xcd * per_xcd + (R.map == 1u ? li * n_waves + wave : wave * (gridDim.x >> 3) + li);
        }
        // map 3: every wave CLAIMS its next partition of the pass from one counter (what would dynamic balancing buy? XCDs do
        // not stream equally fast when all of them ask for all they can take: tools/batch_trace.py)
        const bool dyn = R.map == 3u;
        auto claim_next = [&]() -> uint32_t {
            uint32_t v = 0u;
            if (lane == 0) v = atomicAdd(&R.claim[32u * pass], 1u);
            return __builtin_amdgcn_readfirstlane(v);
        };
        if (dyn) p_first = claim_next();
        for (uint32_t p = p_first; p < R.n_parts; p = dyn ? claim_next() : p + n_waves * gridDim.x) {
            const uint32_t first = R.part_first[p], count = R.part_count[p];
            const uint8_t *pk = base + (size_t)first * PB;
            if (WORK < 0) {  // the engine's own per-packet arithmetic (x gathers from LDS, products, segmented scan) on a ring of DEPTH
                if constexpr (BPL == 24) {
                    Pkt<4, VT_F32> buf[DEPTH];
#pragma unroll
                    for (int j = 0; j < DEPTH - 1; ++j) load_packet<4, VT_F32>(pk + (size_t)((uint32_t)j < count ? j : count - 1u) * PB, lane, buf[j]);
                    float carry = 0.0f, best = 0.0f;
                    for (uint32_t i = 0; i < count; i += DEPTH) {
#pragma unroll
                        for (int j = 0; j < DEPTH; ++j) {
                            const uint32_t nxt = i + j + DEPTH - 1;
                            load_packet<4, VT_F32>(pk + (size_t)(nxt < count ? nxt : count - 1u) * PB, lane, buf[(j + DEPTH - 1) % DEPTH]);
                            if (i + j < count) {
                                const Reduced<4> S = reduce_packet<4, QM_F32>(buf[j], carry, lds_addr_of(xl), 0u);
                                const float trig = trigger_of<4, false>(S);
                                if (WORK == -1) best = fmaxf(best, trig);
                                else if (__any(trig >= 1e30f)) best += S.S;  // WORK == -2: the hot-path trigger as the engine has it
                            }
                        }
                    }
                    acc ^= __float_as_uint(best) ^ __float_as_uint(carry);
                }
            } else if (WORK == 0) {
                uint32_t i = 0;
                const uint32_t tpkt_fp = (R.period != 0u && count != 0u) ? (uint32_t)((float)R.period / (float)count) : 0u;
                if (tpkt_fp != 0u && pass == 0u && p == p_first) sched_fp = (uint32_t)__builtin_amdgcn_s_memrealtime() << 8;
                for (; i + DEPTH <= count; i += DEPTH) {
#pragma unroll
                    for (int j = 0; j < DEPTH; ++j) acc ^= read_probe_packet<BPL>(pk + (size_t)(i + j) * PB, lane);
                    if (tpkt_fp != 0u) {  // (polled: the probe has no arithmetic to hide the clock's answer behind, and nothing else to do)
                        sched_fp += tpkt_fp * (uint32_t)DEPTH;
                        while ((int32_t)(sched_fp - ((uint32_t)__builtin_amdgcn_s_memrealtime() << 8)) > (int32_t)(8u << 8)) __builtin_amdgcn_s_sleep(4);
                    }
                }
                for (; i < count; ++i) acc ^= read_probe_packet<BPL>(pk + (size_t)i * PB, lane);
                if (tpkt_fp != 0u) sched_fp += tpkt_fp * (count % (uint32_t)DEPTH);
            } else {  // a rotating window of DEPTH requests, WORK dependent multiply-adds on every packet as it arrives
                uint32_t buf[DEPTH];
#pragma unroll
                for (int j = 0; j < DEPTH; ++j) buf[j] = (uint32_t)j < count ? read_probe_packet<BPL>(pk + (size_t)j * PB, lane) : 0u;
                for (uint32_t i = 0; i < count; i += DEPTH) {
#pragma unroll
                    for (int j = 0; j < DEPTH; ++j) {
                        uint32_t w = buf[j];
                        const uint32_t nxt = i + j + DEPTH;
                        buf[j] = nxt < count ? read_probe_packet<BPL>(pk + (size_t)nxt * PB, lane) : 0u;
#pragma unroll
                        for (int t = 0; t < WORK; ++t) w = (w ^ 0x9E3779B1u) + acc;  // v_xad_u32: full-rate, dependent
                        acc ^= (i + j < count) ? w : 0u;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc ^= (uint32_t)__shfl_xor((int)acc, d);
    if (lane == 0) R.sink[blockIdx.x * n_waves + wave] = acc;
    if (lane == 0 && R.t_end) R.t_end[blockIdx.x * n_waves + wave] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace tkspmv
