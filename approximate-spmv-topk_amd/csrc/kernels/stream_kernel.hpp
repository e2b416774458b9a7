// kernels/stream_kernel.hpp -- stream_kernel: one query per launch (fused selection tail, deferred selection, or SpMV-only scores).
// Part of engine.hip (one translation unit: included there in this order; device code only).
#pragma once
#include <cstddef>
#include "packet_math.hpp"

namespace tkspmv {

#ifndef TKSPMV_STREAM_TURNS
#define TKSPMV_STREAM_TURNS 2
#endif
#ifndef TKSPMV_STREAM_PRIO
#define TKSPMV_STREAM_PRIO 2
#endif
#ifndef TKSPMV_REDUCER_SLEEP
#define TKSPMV_REDUCER_SLEEP 8
#endif
constexpr unsigned long long FLUSH_TAU_WAIT = 2000;  // x 10 ns: longest wait of a wave for a first threshold
#ifndef TKSPMV_DEFER_PACKETS
#define TKSPMV_DEFER_PACKETS 2
#endif
constexpr int DEFER = TKSPMV_DEFER_PACKETS;  // packets per wave whose rows are judged at the end (threshold exchange cold start)

// One static LDS object per workgroup. x sits at LDS offset 0, so that (column word & 0xFFFC) IS the ds_read address;
// the selection tail reuses the bytes of x and of the candidate list, which are dead by then. Static objects are
// addressed with ds_* instructions for certain: a pointer carved out of the dynamic region can degrade to flat_*
// accesses, and one flat access in the loop forces s_waitcnt vmcnt(0), draining the packet prefetch every iteration.
template <int XCOLS>
struct StreamLds {
    union {
        struct {
            float x[XCOLS];
            uint2 cand[ListGeom<XCOLS>::CAND_CAP];  // private candidate lists {score bits, row}
        } w;
        SelectShared sel;  // fused selection tail (last workgroup only)
    } u;
    uint32_t misc[MISC_WORDS];
};

#ifndef TKSPMV_NBUF
#define TKSPMV_NBUF 3
#endif
// DBG = false (production): tracing / statistics / ablation hooks compiled out (see batch_kernel).
template <int C, bool SCORES, int XCOLS, int QM = QM_F32, int NBUF = TKSPMV_NBUF, bool DBG = false>
__global__ void __launch_bounds__(576, ((C == 8 && !SCORES) || QM == QM_F32C12) ? 6 : 5) stream_kernel(const StreamParams P, const SelectParams SP) {
    constexpr bool FILT = false;  // (every use of F below is compiled out)
    const FilterParams F{};
#include "stream_body.hpp"
}

// Filtered top-k (tkspmv_enqueue_filtered): stream_kernel restricted to the rows the allow-mask F admits. Masked rows are marked
// right after expand(), like placeholders of empty rows, so neither a candidate list nor a published group maximum ever holds
// one (the threshold stays a lower bound of the k-th ELIGIBLE score); the SpMV-only variant writes -inf for them. The mask words
// of a packet's first rows are scalar loads issued one packet ahead (mask_pair): lgkmcnt, never the packet loads' vmcnt.
template <int C, bool SCORES, int XCOLS, int QM = QM_F32, int NBUF = TKSPMV_NBUF>
__global__ void __launch_bounds__(576, ((C == 8 && !SCORES) || QM == QM_F32C12) ? 6 : 5)
    stream_filter_kernel(const StreamParams P, const SelectParams SP, const FilterParams F) {
    constexpr bool FILT = true;
    constexpr bool DBG = false;
#include "stream_body.hpp"
}

}  // namespace tkspmv
