// engine.hip -- fused Top-K SpMV for MI355X (gfx950, wave64). Hand-written HIP; no MFMA (there is no dense
// contraction on this path), HBM-streaming bound.
//
// Replaces the reference's FPGA kernel spmv_bscsr_top_k_main (src/fpga/src/ip/spmv/
// spmv_bscsr_top_k_multicore.cpp:8-186, .hpp:104-504: scatter -> aggregation -> summary -> top-k update) and the
// GPU baseline's cusparseSpMV + thrust::sort_by_key + get_topk (src/gpu/host_spmv_topk_csr_gpu.cu:171-231) with
//
//   stream_kernel : one wave per row partition streams wave-BSCSR packets (wbscsr.hpp); x lives in LDS; per
//                   packet: gather x, multiply, in-lane segmented sums, cross-lane segmented scan, one compare
//                   of the lane's best finished row against the running threshold tau. Rows that pass are
//                   appended to a per-workgroup candidate list in LDS (rare). No N-vector is written.
//   tau           : every workgroup publishes the best score it has seen (one u32 per group, single writer).
//                   The published maxima are scores of distinct rows, so the k-th largest of them is a valid lower
//                   bound of the global k-th best score and rows below it can be dropped. Stale or missing values
//                   only make tau smaller: correctness never depends on inter-workgroup timing, only the
//                   candidate count does. All exchange traffic is issued by one "server" wave per workgroup.
//   select tail   : (last workgroup to finish, or select_kernel) exact top-k of the surviving candidates, ordered (score desc, row desc) = sort_tuples
//                   (src/common/utils/evaluation_utils.hpp:40-62); pads with (0, 0.0f) like the gold's
//                   zero-initialised list (gold_algorithms.hpp:203-206).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <string>
#include <vector>

#include "device_pack.hpp"
#include "engine.hpp"
#include "host_utils.hpp"
#include "options.hpp"
#include "stream_format.hpp"
#include "wsell.hpp"

#include "kernels/common.hpp"
#include "kernels/select.hpp"
#include "kernels/packet_math.hpp"
#include "kernels/stream_kernel.hpp"
#include "kernels/local.hpp"
#include "kernels/batch_kernel.hpp"
#include "kernels/multi_kernel.hpp"
#include "kernels/radix_select.hpp"
#include "kernels/read_probe.hpp"
#include "kernels/range_kernel.hpp"
#include "kernels/facet_kernel.hpp"
#include "kernels/match_kernel.hpp"
#include "kernels/row_vectors.hpp"
#include "kernels/score_rows.hpp"
#include "kernels/row_stats.hpp"
#include "kernels/assign.hpp"
#include "kernels/nearest.hpp"
#include "kernels/col_stats.hpp"
#include "kernels/label_sums.hpp"
#include "kernels/group_select.hpp"
#include "kernels/after_select.hpp"
#include "kernels/boost_cut.hpp"
#include "kernels/boost_forms.hpp"

namespace tkspmv {

// Empty kernel with the stream kernel's geometry: calibrates what an event bracket adds around one launch.
__global__ void __launch_bounds__(576) null_kernel(const uint32_t *p) {
    if (p == nullptr && threadIdx.x == 123456u) __builtin_trap();
}

// What a KERNEL sees of words the CPU stored into device memory through the PCIe BAR (tkspmv_create's check of the BAR path of
// tkspmv_set_query): plain loads, through the same caches a streaming kernel's loads of x go through.
__global__ void bar_check_kernel(const uint32_t *x, uint32_t last, uint32_t *out) {
    if (threadIdx.x == 0) {
        out[0] = x[0];
        out[1] = x[last];
    }
}

// ------------------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------------------
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            err = std::string(#expr) + " failed: " + hipGetErrorString(_e);                             \
            return TKSPMV_ERR_DEVICE;                                                                   \
        }                                                                                               \
    } while (0)

// The failure return of the creation stages and of the entry points' argument checks.
static int fail(std::string &err, int status, std::string msg) { err = std::move(msg); return status; }

// Exchange words that other XCDs poll (published maxima, threshold word, tickets) live in fine-grained device memory:
// it is not cached in the per-XCD L2s, so a poll never hits a stale copy (with ordinary memory an agent-scope load can
// keep returning the old value until the line happens to be evicted: milliseconds on an idle L2).
static hipError_t malloc_exchange(void **p, size_t bytes) {
    if (hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained) == hipSuccess) return hipSuccess;
    if (opt("DEBUG_OCC")) fprintf(stderr, "[tkspmv] fine-grained allocation unavailable, using hipMalloc\n");
    (void)hipGetLastError();
    return hipMalloc(p, bytes);
}
enum class Mem { Device, Exchange, Pinned };  // EngineImpl::alloc: hipMalloc, malloc_exchange, hipHostMalloc (mapped)

// The kernels of one engine, chosen once (choose_kernels, at creation) by the format of its packet stream. NULL: the family has no
// kernel for this format. multi_kernel is keyed on the ELL copy's value type and the queries per pass (choose_kernels too);
// read_probe_kernel keeps its own table: its option is read per call.
typedef void (*stream_fn)(const StreamParams, const SelectParams);
typedef void (*filter_fn)(const StreamParams, const SelectParams, const FilterParams);
typedef void (*range_fn)(const StreamParams, const RangeParams);
typedef void (*facet_fn)(const StreamParams, const FacetParams);
typedef void (*match_fn)(const StreamParams, const MatchParams);
typedef void (*row_vectors_fn)(const RowVecParams);
typedef void (*score_rows_fn)(const ScoreRowsParams);
typedef void (*row_stats_fn)(const StreamParams, const RowStatsParams);
typedef void (*col_stats_fn)(const StreamParams, const ColStatsParams);
typedef void (*assign_fn)(const StreamParams, const AssignParams);
typedef void (*nearest_fn)(const StreamParams, const NearestParams);
typedef void (*label_sums_fn)(const StreamParams, const LabelSumsParams);
typedef void (*batch_fn)(const BatchArgs);
typedef void (*single_fn)(const StreamParams, const SelectParams, const LocalParams);
typedef void (*multi_fn)(const StreamParams, const SelectParams, const MultiParams);
struct Kernels {
    stream_fn stream[2] = {};  // [SCORES]; [0] is the tracing twin on an engine that traces
    filter_fn filter[2] = {};  // [SCORES]
    range_fn range[2] = {};    // [FILT]
    facet_fn facet[2] = {};    // [FILT]
    match_fn match[2] = {};    // [FILT]
    row_vectors_fn row_vectors = nullptr;
    score_rows_fn score_rows = nullptr;  // (no x in LDS: one instantiation serves every column tier)
    row_stats_fn row_stats[4] = {};      // [kind: TKSPMV_ROW_NNZ .. TKSPMV_ROW_INV_L2] (no x at all: likewise)
    col_stats_fn col_stats[2][2] = {};   // [EXT: TKSPMV_COL_MAX / _MIN][FILT]
    assign_fn assign = nullptr;          // (16384 / XCOLS vectors in LDS per pass)
    nearest_fn nearest[3] = {};          // [lists of 1, 2, 4 entries] (the same vectors per pass)
    label_sums_fn label_sums[2] = {};    // [LDS_SINK]; [1] NULL at the 16384-column tier (8192 / XCOLS bins in LDS per launch)
    batch_fn batch[2] = {};    // [LOCAL: the kernel of the checked local thresholds]; the tracing twins likewise
    single_fn single = nullptr;
    multi_fn multi = nullptr;  // multi-query engines only
};
// Packet buffers of match_kernel. Its loads are 8 bytes per lane (16 at 8 entries), so more than range_kernel's 3 cost few registers;
// builds with 3, 6 and 8 came out within 4 % of this one, less than the yardstick drifted between them ("Packets in
// flight"): no count is shown to pay.
#ifndef TKSPMV_MATCH_NBUF
#define TKSPMV_MATCH_NBUF 4
#endif
// The instantiations of ONE format, every family restricted to the formats it is built for (the predicates of stream_format.hpp).
template <int C, int XCOLS, int QM>
static Kernels kernels_of(bool dbg) {
    constexpr StreamFormat F{C, XCOLS, QM};
    constexpr int NBUF = C == 8 ? 2 : TKSPMV_NBUF;  // (8 entries per lane: two packet buffers, 3 KB packets)
    Kernels K;
    K.stream[0] = &stream_kernel<C, false, XCOLS, QM, NBUF>;
    K.stream[1] = &stream_kernel<C, true, XCOLS, QM, NBUF>;
    if constexpr (is_fp32(F)) {
        K.filter[0] = &stream_filter_kernel<C, false, XCOLS, QM, NBUF>;
        K.filter[1] = &stream_filter_kernel<C, true, XCOLS, QM, NBUF>;
        K.range[0] = &range_kernel<C, XCOLS, QM, false, C == 8 ? 2 : 3>;
        K.range[1] = &range_kernel<C, XCOLS, QM, true, C == 8 ? 2 : 3>;
        K.facet[0] = &facet_kernel<C, XCOLS, QM, false, C == 8 ? 2 : 3>;
        K.facet[1] = &facet_kernel<C, XCOLS, QM, true, C == 8 ? 2 : 3>;
        K.match[0] = &match_kernel<C, XCOLS, QM, false, TKSPMV_MATCH_NBUF>;
        K.match[1] = &match_kernel<C, XCOLS, QM, true, TKSPMV_MATCH_NBUF>;
        K.row_vectors = &row_vectors_kernel<C, XCOLS, QM == QM_F32C12>;
        K.score_rows = &score_rows_kernel<C, QM == QM_F32C12>;
        K.row_stats[TKSPMV_ROW_NNZ] = &row_stats_kernel<C, QM == QM_F32C12, ROW_STAT_NNZ>;
        K.row_stats[TKSPMV_ROW_L1] = &row_stats_kernel<C, QM == QM_F32C12, ROW_STAT_L1>;
        K.row_stats[TKSPMV_ROW_L2SQ] = &row_stats_kernel<C, QM == QM_F32C12, ROW_STAT_L2SQ>;
        K.row_stats[TKSPMV_ROW_INV_L2] = &row_stats_kernel<C, QM == QM_F32C12, ROW_STAT_INV_L2>;
        K.assign = &assign_kernel<C, XCOLS, QM>;
        K.nearest[0] = &nearest_kernel<C, XCOLS, QM, 1>;
        K.nearest[1] = &nearest_kernel<C, XCOLS, QM, 2>;
        K.nearest[2] = &nearest_kernel<C, XCOLS, QM, 4>;
        K.col_stats[0][0] = &col_stats_kernel<C, XCOLS, QM == QM_F32C12, false, false>;
        K.col_stats[0][1] = &col_stats_kernel<C, XCOLS, QM == QM_F32C12, false, true>;
        K.col_stats[1][0] = &col_stats_kernel<C, XCOLS, QM == QM_F32C12, true, false>;
        K.col_stats[1][1] = &col_stats_kernel<C, XCOLS, QM == QM_F32C12, true, true>;
        K.label_sums[0] = &label_sums_kernel<C, XCOLS, QM == QM_F32C12, false>;
        if constexpr (label_sums_lds_bins(XCOLS) != 0u) K.label_sums[1] = &label_sums_kernel<C, XCOLS, QM == QM_F32C12, true>;
    }
    if constexpr (is_batchable(F)) {
        K.batch[0] = &batch_kernel<C, XCOLS, QM, false, false>;
        K.batch[1] = &batch_kernel<C, XCOLS, QM, false, true>;
    }
    if constexpr (has_tracing_twins(F)) {
        if (dbg) {
            K.stream[0] = &stream_kernel<C, false, XCOLS, QM, NBUF, true>;
            K.batch[0] = &batch_kernel<C, XCOLS, QM, true, false>;
            K.batch[1] = &batch_kernel<C, XCOLS, QM, true, true>;
        }
    }
    if constexpr (has_single_kernel(F)) K.single = &single_kernel<QM>;
    return K;
}
static Kernels kernels_for(StreamFormat f, bool dbg) {
#define X(C, XCOLS, QM) \
    if (f.c == C && f.xcols == XCOLS && f.qm == QM) return kernels_of<C, XCOLS, QM>(dbg);
    TKSPMV_STREAM_FORMATS(X)
#undef X
    return Kernels{};
}

// The waves keep a timetable in 32 bits of ticks (10 ns) << 8, 168 ms to the wrap: a period of ns per query in those units ...
static uint32_t period_units(uint64_t ns) { return (uint32_t)std::min<uint64_t>(0xFFFFFF00ull, ns * 256u / 10u); }
// ... and whether a launch of n queries could last a quarter of the wrap (32 queries of 1.3 ms: 80M rows). Such a launch keeps no
// timetable (the batch kernel paces by rank instead).
static bool outlasts_timetable(uint32_t period_ns, int n) { return (uint64_t)period_ns * (uint64_t)n > 40000000ull; }

// One engine. What the whole engine shares comes first: the descriptor, the packed matrix's host-side tables, the device, the
// record of its buffers, its stream and events, the launch geometry, the stream format and its kernels. Everything else belongs to
// ONE launch path and sits in that path's group below; each group says which creation stage (create_impl) fills it and who changes
// it afterwards. The launch methods follow the groups: a method that is const changes nothing.
struct EngineImpl {
    tkspmv_desc desc{};
    PackedMatrix pm;  // host copy is dropped after upload (only the small tables are kept)
    tkspmv_info info{};
    int device = 0;
    // Every device and pinned buffer of the engine, each once: ~Engine frees what is recorded here. (Views into a recorded
    // buffer -- st[1..], d_replicas[0], the device side of a mapped block -- are not recorded.)
    struct Owned { void *p; bool pinned; };
    std::vector<Owned> owned;
    // Allocates, fills with the byte `fill` unless it is negative, and records; *p is left alone if the allocation fails.
    template <class T>
    hipError_t alloc(T *&p, size_t bytes, Mem kind = Mem::Device, int fill = -1, unsigned host_flags = hipHostMallocMapped | hipHostMallocCoherent) {
        void *q = nullptr;
        hipError_t e = kind == Mem::Pinned ? hipHostMalloc(&q, bytes, host_flags) : kind == Mem::Exchange ? malloc_exchange(&q, bytes) : hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        owned.push_back({q, kind == Mem::Pinned});
        p = static_cast<T *>(q);
        if (fill >= 0 && kind == Mem::Pinned) std::memset(q, fill, bytes);
        else if (fill >= 0) e = hipMemset(q, fill, bytes);
        return e;
    }
    template <class T> T *adopt(T *p) {  // a device buffer allocated elsewhere (the device packers)
        if (p) owned.push_back({p, false});
        return p;
    }
    void release(const void *p) {  // frees a recorded buffer before ~Engine (NULL or unrecorded: nothing)
        const auto it = std::find_if(owned.begin(), owned.end(), [p](const Owned &b) { return b.p == p; });
        if (!p || it == owned.end()) return;
        (void)(it->pinned ? hipHostFree(it->p) : hipFree(it->p));
        owned.erase(it);
    }
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;  // (ev0, ev1: the brackets of the measurements; ev2: behind the upload of x)
    uint32_t grid = 0, block = 0;
    StreamFormat fmt{};  // what the kernels of this engine's packet stream are instantiated with (exchange_geometry)
    Kernels kern;        // ... and those kernels (choose_kernels)

    // The matrix in HBM: the wave-BSCSR packet stream, its row and partition tables, the stream's extra copies. Filled by
    // pack_matrix (the device packer's buffers, the uniform table) and upload_matrix; afterwards only launch_counter moves: every
    // launch method that streams advances it by its queries, so that consecutive queries read consecutive copies.
    struct Matrix {
        uint8_t *d_packets = nullptr;
        std::vector<uint8_t *> d_replicas;  // extra copies of the packet stream (cache-defeat mode)
        uint64_t launch_counter = 0;
        uint32_t *d_pkt_row = nullptr, *d_part_first = nullptr, *d_part_count = nullptr;
        uint32_t uni_ppp = 0, uni_last = 0;  // uniform partition table (StreamParams::uni_ppp): partition q = packets [q * uni_ppp, ...)
        const uint8_t *packets(uint64_t n) const { return d_replicas.empty() ? d_packets : d_replicas[n % d_replicas.size()]; }  // the copy query n streams
        // The batch kernel's own copies (compact_stream; empty: it streams the canonical ones): the same packets re-encoded at 5 bytes
        // per entry (wbscsr.hpp F32E5), as many copies as the canonical stream has. Every other kernel reads the canonical stream.
        std::vector<uint8_t *> d_compact;
        uint32_t compact_top4 = 0;  // bits 31..28 of every fp32 word of the matrix (StreamParams::top4)
        bool compact() const { return !d_compact.empty(); }
        const uint8_t *batch_packets(uint64_t n) const { return compact() ? d_compact[n % d_compact.size()] : packets(n); }  // what query n of the batch path streams
        uint32_t batch_packet_bytes(const PackedMatrix &pm) const { return compact() ? F32E5_PACKET_BYTES : pm.packet_bytes; }
    } mat;

    // The host boundary of the reference loop (reset -> operator() -> read_result, host_spmv_bscsr.cpp:602-632) and the engine's own
    // result pair. set_query copies x into pinned host memory and enqueues the 4 KiB upload without waiting for it -- or, with a
    // large BAR (bar_x; every MI355X server has it, checked at create), writes x into device memory with plain CPU stores through
    // the PCIe aperture: 0.5 us, no copy kernel ahead of the query's launch --; run() launches the fused kernel, whose selection
    // tail also writes the k results and an epoch flag to pinned host memory, and polls that flag; read() copies from the pinned
    // block. No stream synchronisation, no device-to-host copy on the critical path. Filled by setup_host_boundary; changed by
    // the entry points: set_query* (the installed vector), run (epoch, x_pending) and whatever writes a result pair (ran,
    // last_on_host).
    struct HostBoundary {
        float *d_x = nullptr;
        const float *d_x_cur = nullptr;
        float *h_x = nullptr;            // pinned staging copy of x
        float *h_x_dev = nullptr;        // h_x as the device sees it (TKSPMV_HOST_X=direct: kernels read x from host memory)
        bool host_x_direct = false;
        uint32_t *h_res = nullptr;       // pinned: [k] row ids, [k] score bits, [2k] epoch flag
        uint32_t *h_res_dev = nullptr;   // the same block as the device sees it
        uint32_t host_epoch = 0;
        bool last_on_host = false;       // the most recent result is complete in h_res
        bool x_pending = false;          // an upload from h_x may still be in flight
        bool bar_x = false;
        // CPU stores through the BAR pass the host data path (HDP) on their way to memory: the documented protocol ends them with a
        // write to the device's HDP_MEM_COHERENCY_FLUSH_CNTL register and a read back of it (what ROCclr does behind its own large-BAR
        // copies); the register's address comes from hipDeviceAttributeHdpMemFlushCntl. No address, no BAR path.
        volatile uint32_t *hdp_flush = nullptr;
        void flush_hdp() const {
            __builtin_ia32_sfence();
            *hdp_flush = 1u;
            (void)*hdp_flush;  // (the read completes only behind the posted writes before it)
        }
        int host_path = 1;                  // TKSPMV_HOST_PATH=0: the plain path (stream synchronisation + copies)
        bool run_events = false;            // TKSPMV_RUN_EVENTS=1: tkspmv_run brackets the fused launch with a hipEvent pair instead of taking the kernel's own duration
        unsigned long long *d_tstart = nullptr;  // the fused launch's start stamp (SelectParams::t_start)
        bool have_query = false;
        bool ran = false;
        uint32_t *d_out_idx = nullptr;      // the engine-owned result pair ("engine buffers, the last query wins")
        float *d_out_val = nullptr;
        void result_on_device() {  // an entry point has enqueued queries that write a result pair: tkspmv_read goes to the device
            ran = true;
            last_on_host = false;
        }
    } host;

    // Exchange state of the queries in flight (published maxima, threshold word, survivor slots, overflow list), one set per
    // query: with deferred selection, launch q+1 streams into one set while its workgroup 0 selects query q from the other; the
    // batch kernel runs one set per query of a launch; everything else uses set 0. The geometry comes from exchange_geometry, the
    // buffers from setup_exchange_sets (d_done: setup_host_boundary); nothing here changes after creation.
    struct ExchangeSets {
        struct ExState {
            uint32_t *tau_g = nullptr, *gmax = nullptr, *ovf_count = nullptr;
            unsigned long long *wg_cand = nullptr, *ovf = nullptr;
            float *unit_inv = nullptr;
        };
        static constexpr int N_STATE = BATCH_MAX;  // deferred selection uses sets 0/1, the batch kernel one per query
        static constexpr uint32_t GMAX_WORDS = MAX_GM * 64, STATE_WORD_STRIDE = 64;  // set-to-set distances (elements)
        ExState st[N_STATE];
        uint32_t n_sets = 0, gpw = 1, n_groups_pub = 0, cand_cap = 0, lds_bytes = 0;
        uint32_t groups_with_rows = 0;  // publishing groups that own at least one wave partition
        uint32_t ovf_cap = 0;
        uint32_t ovf_lists = 1;         // overflow lists allocated (batch engines: 4, or 2 with local thresholds; shared by the queries of a launch under flow control)
        uint32_t *d_ovf_epoch = nullptr;  // [ovf_lists] x 32 words: the epoch words of the overflow lists' flow control
        uint32_t *d_done = nullptr;
    } ex;

    // One query per launch: the selection fused into the stream kernel's tail, or deferred -- the selection of a back-to-back
    // query runs inside the NEXT deferred launch (or in drain()). fused / can_defer: choose_path. The rest is the selection still
    // owed, moved by launch_deferred and settled by drain, launch_multi and whoever launches next.
    struct Deferred {
        bool fused = true;
        bool can_defer = false;
        int cur_set = 0;                  // set the next deferred launch streams into
        bool pending = false;             // a deferred selection is owed for ...
        int pending_set = 0;              // ... this set, into ...
        uint32_t *pending_idx = nullptr;  // ... these result buffers
        float *pending_val = nullptr;
    } defer;

    // Large k (see radix_hist_kernel): every query = scores kernel + radix select + the selection kernel; with partitions > 1 and
    // k > k_per_partition the reference's lossy per-partition lists instead of the radix select. approx_parts: check_desc; the
    // rest: choose_path. Unchanged afterwards.
    struct Radix {
        bool use_radix = false;
        bool approx_parts = false;
        float *d_rscores = nullptr;   // [rows], -inf where a row has no entry (never written by the scores kernel)
        uint32_t *d_rhist = nullptr;  // [4][256]
    } radix;

    // Multi-query passes (multi_kernel, desc.multi_q): fp32 values, <= 1024 columns, exchange on. multi_q queries share one pass
    // over the wave-sliced ELL copy of the matrix (wsell.hpp); a group's selection is owed to the next launch of its chain (or to
    // drain()). Two independent chains of launches (TKSPMV_MULTI_CHAINS=1 switches the second off): chain c runs on its own
    // stream with its own exchange-state sets [16c, 16c + 16), its groups alternating between the halves of those, so the start-up
    // of one chain's launch fills the tail of the other's. Filled by setup_multi; launch_multi moves the owed groups and the
    // halves, tkspmv_time_multi sums the STATS figures.
    struct Multi {
        bool can_multi = false;
        int multi_q = 0;
        int multi_group = 0;  // queries per multi-query LAUNCH (= its selector workgroups): multi_q, or with one query per pass up to MULTI_Q_MAX passes
        uint8_t *d_sell_packets = nullptr;
        std::vector<uint8_t *> d_sell_replicas;
        uint32_t *d_sell_rows = nullptr, *d_sell_part_first = nullptr, *d_sell_part_count = nullptr, *d_sell_part_slice0 = nullptr;
        uint32_t sell_parts = 0, multi_stream_waves = 8, sell_packet_bytes = 1536;
        MultiGroup pending_group[2]{};  // per chain: the group whose selection is owed
        int half[2] = {0, 0};           // per chain: the half of its sets the next launch streams into
        int multi_chains = 2;
        hipStream_t side = nullptr;     // the second chain's stream
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        uint32_t *d_multi_out_idx = nullptr;  // [2 * MULTI_Q_MAX][k] results of tkspmv_time_multi
        float *d_multi_out_val = nullptr;
        uint64_t multi_stat_queries = 0, multi_waits = 0, multi_wait_ticks = 0, multi_rows_offered = 0, multi_rows_overflowed = 0;  // option STATS, summed over tkspmv_time_multi calls
        const uint8_t *packets(uint64_t n) const { return d_sell_replicas.empty() ? d_sell_packets : d_sell_replicas[n % d_sell_replicas.size()]; }  // the copy pass n streams
    } multi;

    // Launches of the batch kernel: up to batch_max queries each, one exchange-state set per query. can_batch: choose_path;
    // n_sel_wg: setup_geometry; tickets: setup_verdicts; batch_max, the workgroups' records and the alias pair:
    // setup_exchange_sets. batch_args counts the launches. The ext_* words are tkspmv_time_queries' hand-over of its bracket: the
    // events ride on the region's first and last kernel (hipExtLaunchKernelGGL: the dispatch's own start and end stamps -- what
    // rocprofv3 reports) instead of being recorded around them; time_queries sets them, launch_sequence marks the last launch,
    // launch_batch takes them.
    struct Batch {
        bool can_batch = false;         // batch kernel usable (exchange on, x double-buffered in LDS: is_batchable)
        int batch_max = BATCH_MAX;      // queries per launch = exchange-state sets allocated (option BATCH_MAX)
        uint32_t n_sel_wg = 1;          // selector workgroups of a batch launch (BatchParams::n_selectors): 4 on small matrices
        uint32_t *d_tickets = nullptr;  // [BATCH_MAX] x 32 words
        unsigned long long *d_rec_slots = nullptr;  // [BATCH_MAX][grid][WG_SLOTS] the workgroups' records of local mode
        uint32_t *d_rec_used = nullptr;             // [BATCH_MAX][grid]
        uint32_t *d_alias_idx = nullptr;  // [BATCH_MAX][k] where the earlier queries of a launch write when they share the last one's buffer
        float *d_alias_val = nullptr;
        uint64_t batch_launches = 0;
        hipEvent_t ext_start = nullptr, ext_stop = nullptr;
        bool ext_last = false;    // (launch_sequence: the launch_batch being made is the region's last)
        bool ext_record = false;  // the same two events RECORDED right in front of the first and right behind the last launch (EXT_EVENTS=2)
    } batch;

    // Who looks at the verdict of a launch of checked local thresholds. The kernel's verdict words, and the host's side of them
    // (BatchParams::verdict_host): a ring of host-visible words, one per batch launch on the engine's own stream, and the launches
    // whose word has not been looked at yet. While the verdicts the host has SEEN are clean, a local launch goes out alone and
    // settle() -- called wherever the host has just waited for the engine's stream -- repairs what a check flagged after all (an
    // exact launch of the flagged queries, then one more wait). An observed failure puts the in-stream repair launch back behind
    // the next DISTRUST_LAUNCHES launches (it also keeps the gate's books). Launches on a caller's stream are never trusted: nobody
    // tells the engine when the caller has waited. Filled by setup_verdicts; launch_batch queues the checks and counts,
    // settle() looks at them and moves the trust, autotune_pacing resets both.
    struct Trust {
        static constexpr uint32_t VERDICT_RING = 8192, DISTRUST_LAUNCHES = 64;  // (launches the host may enqueue between two waits and still look at every verdict)
        unsigned long long *d_verdict = nullptr;  // four words of 128 bytes: a launch zeroes the word of the launch after the next
        unsigned long long *h_verdict = nullptr, *h_verdict_dev = nullptr;
        struct PendingCheck {
            BatchArgs A;
            uint32_t slot;
            bool trusted;  // no repair launch went out behind it
        };
        std::deque<PendingCheck> pending_checks;
        uint64_t verdict_seq = 0, late_repairs = 0, trusted_launches = 0;
        uint32_t clean_seen = 0, distrust_left = 0;
        bool repair_by_host = true;  // option REPAIR=stream: the exact launch always follows in the stream
        bool has_room() const { return h_verdict && pending_checks.size() + 1u < VERDICT_RING; }  // the host can watch one more launch
        bool trusts() const { return repair_by_host && clean_seen != 0u && distrust_left == 0u; }  // a watched launch goes out alone
    } trust;

    // Workgroup-local thresholds (checked) and the pacing of the launches that stream with them: the modes, the carried priors
    // and their signatures, the pauses by rank and the timetable. Filled by setup_verdicts; autotune_pacing measures the pacing on
    // this box (pace_quads, pace_levels, pace_period_ns, pace_tuned_*) and clears what its launches carried. Unchanged afterwards
    // (the kernels move the device words).
    struct LocalThresholds {
        uint32_t use_local = 0;    // BatchParams::local: 0 off, 1 / 2: a wave's best / second best packet maximum
        uint32_t single_mode = 0;  // the same choice for ONE query per launch (single_kernel): by the failure estimate alone, whatever the size
        float *d_wg_prior = nullptr;  // [grid] + the countdown word (BatchParams::wg_prior / prior_block)
        float *d_wg_sig = nullptr;    // [grid][8] the signatures of the remembered priors and the second prior (BatchParams::wg_sig; option SIGNATURES=0: none)
        float local_beta = 1.0f;
        uint32_t pace_quads = 0, pace_levels = 3, pace_base = 0;  // pacing by rank (BatchParams::pace_quads, pace_levels, pace_base)
        bool pace_carry = true;            // option PACE_CARRY=0: every launch starts unpaced
        uint32_t *d_wg_pace = nullptr;     // [grid] the pause every workgroup ended its last launch with (BatchParams::wg_pace)
        uint32_t *d_pace_adapt = nullptr;  // [0] what launches add to the period, [1] late waves of the launch in flight (BatchParams::pace_adapt)
        bool pace_adapt_on = true;         // option PACE_ADAPT=0: the period stays what tkspmv_create measured
        uint32_t pace_period_ns = 0;       // pacing by the clock (BatchParams::pace_period): ns per query of every wave's timetable; 0: pacing by rank
        uint32_t pace_tuned_us = 0;        // 0: the pacing is the static default (or an option); else what tkspmv_create's measurement took
        uint32_t pace_tune_launches = 0;   // ... and the batch launches it made (synthetic queries: a kernel trace of a run holds them)
    } local;

    // single_kernel (kernels/local.hpp): the launch of tkspmv_run on engines that stream with workgroup-local thresholds. Filled
    // by setup_single; launch_single counts the launches, tkspmv_run the repairs.
    struct Single {
        bool can_single = false;
        unsigned long long *d_lslots = nullptr;  // [grid][WG_SLOTS] the workgroups' records
        uint32_t *d_lused = nullptr;             // [grid]
        float *d_lprior = nullptr;               // [grid] carried thresholds | 32 words: the suspension counters (LocalParams::prior_block)
        uint32_t *d_lstatus = nullptr;           // [0] 1: the last single launch failed its check
        uint32_t *d_lready = nullptr;            // [grid] the streaming workgroups' flags (LocalParams::ready; NULL: the last workgroup selects)
        uint64_t single_launches = 0, single_repairs = 0;
    } single;

    // Filtered queries (tkspmv_enqueue_filtered, stream_filter_kernel): the allow-mask tkspmv_set_filter installed, ceil(rows / 32)
    // words, and whether one is installed now. No creation stage: tkspmv_set_filter allocates on its first call and is the only writer.
    struct Filter {
        uint32_t *d_filter = nullptr;
        bool have_filter = false;
    } filter;
    uint32_t mask_words() const { return std::max<uint32_t>(1u, (desc.rows + 31u) / 32u); }

    // Range queries (tkspmv_enqueue_range, range_kernel) touch no other group but the matrix. The timetable's period (option
    // RANGE_PERIOD, ns per query, read by setup_verdicts; unset: the engine's own pace_period_ns) and the scratch of
    // tkspmv_run_range, which allocates it on its first call and grows it to the largest capacity asked for.
    struct Range {
        static constexpr int RANGE_MAX = 32;  // queries per launch
        bool range_period_set = false;
        uint32_t range_period_ns = 0;
        uint32_t *d_range_idx = nullptr;
        float *d_range_val = nullptr;
        uint32_t range_cap = 0;
        uint32_t *d_range_word = nullptr;  // [0] the threshold, [1] the count; tkspmv_run_facets: [2] its threshold, [3] its total
        // Facet counts (tkspmv_enqueue_facets, facet_kernel) share the range path's scope, timetable and contract. The bins of the
        // workgroup-private histogram in LDS (option FACET_LDS_BINS, read by setup_verdicts; unset: the column tier's capacity;
        // 0: global atomics always), and the scratch of tkspmv_run_facets, grown to the largest n_groups asked for.
        uint32_t facet_lds_bins = 0;
        uint32_t *d_facet_counts = nullptr;
        tkspmv_facet_best *d_facet_best = nullptr;
        uint32_t facet_cap = 0;
    } range;

    // Term predicates (tkspmv_enqueue_match, match_kernel) touch no other group but the matrix. The scratch of tkspmv_run_match,
    // which allocates it on its first call: the clause table (cols words), the predicate (4 words) and the count (1 word) in one
    // buffer, and the mask it produces (mask_words() words).
    struct Match {
        static constexpr int MATCH_MAX = 32;  // queries per launch
        uint32_t *d_match_in = nullptr;   // [cols] table | [4] predicate | [1] count
        uint32_t *d_match_out = nullptr;  // [mask_words()]
    } match;

    // Queries by stored row (tkspmv_enqueue_row_vectors, row_vectors_kernel) touch no other group but the matrix either. The
    // scratch of tkspmv_run_similar -- a chunk's row ids, its vectors and its [chunk][k] results --, which allocates it on its
    // first call and grows it to the largest chunk asked for (at most SIMILAR_MAX_ROWS rows and SIMILAR_MAX_BYTES of vectors).
    struct Similar {
        static constexpr uint32_t SIMILAR_MAX_ROWS = 1024;
        static constexpr size_t SIMILAR_MAX_BYTES = (size_t)64 << 20;
        uint32_t *d_sim_rows = nullptr, *d_sim_idx = nullptr;
        float *d_sim_xs = nullptr, *d_sim_val = nullptr;
        uint32_t sim_cap = 0;  // rows the scratch holds
    } similar;

    // Scores of given rows (tkspmv_enqueue_score_rows, score_rows_kernel) touch no other group but the matrix either. The scratch of
    // tkspmv_score_rows -- a chunk's query vectors, its row lists and its [queries][rows] scores --, which allocates it on its first
    // call and grows it to the largest chunk asked for (at most SCORE_MAX_QUERIES queries and SCORE_MAX_BYTES of vectors, and
    // SCORE_MAX_ROWS list entries per query).
    struct ScoreRows {
        static constexpr uint32_t SCORE_MAX_QUERIES = 1024, SCORE_MAX_ROWS = 16384;
        static constexpr size_t SCORE_MAX_BYTES = (size_t)64 << 20;
        float *d_sr_xs = nullptr, *d_sr_scores = nullptr;
        uint32_t *d_sr_rows = nullptr;
        uint32_t sr_q_cap = 0, sr_row_cap = 0;  // queries and list entries per query the scratch holds
    } score;

    // Row statistics (tkspmv_enqueue_row_stats, row_stats_kernel) touch no other group but the matrix either. The scratch of
    // tkspmv_row_stats -- rows floats --, which allocates it on its first call.
    struct RowStats {
        float *d_rs_out = nullptr;  // [rows]
    } stats;

    // Assignment (tkspmv_enqueue_assign, assign_kernel) and nearest-n assignment (tkspmv_enqueue_nearest; nearest_fill_kernel,
    // nearest_kernel) likewise. The scratch of tkspmv_assign and tkspmv_nearest, ONE set for both: each host form waits for its own
    // launches before it returns, so a call never finds the other's launches in flight on it. as_n labels and scores per row, grown to
    // the longest list asked for (tkspmv_assign: 1), and a chunk of vectors that grows to the largest chunk asked for (at most
    // ASSIGN_MAX_BYTES).
    struct Assign {
        static constexpr size_t ASSIGN_MAX_BYTES = (size_t)64 << 20;
        uint32_t *d_as_labels = nullptr;  // [rows][n], n <= as_n
        float *d_as_scores = nullptr;     // [rows][n]
        uint32_t as_n = 0;                // entries per row the two hold, <= TKSPMV_NEAREST_MAX_N
        float *d_as_xs = nullptr;         // [as_cap][cols]
        uint32_t as_cap = 0;              // vectors the chunk holds
    } assign;

    // Label sums (tkspmv_enqueue_label_sums, label_sums_kernel) likewise. The scratch of tkspmv_label_sums, which allocates it on its
    // first call: rows labels, and n_bins * cols sums and floats, which grow to the largest n_bins asked for.
    struct LabelSums {
        uint32_t *d_ls_labels = nullptr;  // [rows]
        int64_t *d_ls_sums = nullptr;     // [ls_cap][cols]
        float *d_ls_out = nullptr;        // [ls_cap][cols]
        uint32_t ls_cap = 0;              // bins the scratch holds
    } lsums;

    // Column statistics (tkspmv_enqueue_col_stats, col_stats_kernel) likewise. The scratch of tkspmv_col_stats -- cols words --, which
    // allocates it on its first call.
    struct ColStats {
        static constexpr int COL_STATS_MAX = 32;  // sets per launch
        uint32_t *d_cs_out = nullptr;  // [cols]
    } cstats;

    // The device words of a path with an array select of its own (d_gwords, d_awords): [4][256] histogram, zeroed per query | word 1024:
    // the path's own counter | the candidate counter | what the selection kernel zeroes behind itself (threshold word, nine tickets)
    struct SelectWords { static constexpr uint32_t W_COUNT = 1056, W_TAU = 1088, W_DONE = 1120, N_WORDS = W_DONE + 9 * 32; };

    // Grouped top-k (tkspmv_enqueue_grouped; group_best_kernel, group_split_kernel, group_ids_kernel) touches no other group but the
    // matrix either: its scores go to an array of its own, its selection runs on its own histogram, candidate list and counters, and
    // the selection kernel gets words of this group where it resets exchange state behind itself. The labels are a property of the
    // index like the allow-mask. No creation stage: tkspmv_set_groups allocates (all of it again when n_groups grows) and is the
    // only writer; the kernels move the device words and leave them zero behind every query.
    struct Grouped {
        bool have_groups = false;
        uint32_t n_groups = 0, group_cap = 0;  // labels installed; groups the per-group buffers hold
        uint32_t *d_groups = nullptr;          // [rows]
        float *d_gy = nullptr;                 // [rows] the scores of the query in flight; -inf where a row has no entry (never written)
        unsigned long long *d_gkey = nullptr;  // [group_cap] best (order key << 32 | row) per group; zero between queries
        float *d_gscore = nullptr;             // [group_cap]
        uint32_t *d_grow = nullptr;            // [group_cap] group -> its representative's row (the selection's pos_to_row)
        unsigned long long *d_gcand = nullptr; // [group_cap] candidate list of the radix filter
        // SelectWords; word 1024 counts the non-empty groups (zeroed in front of every query, with the histogram)
        uint32_t *d_gwords = nullptr;
        static constexpr uint32_t W_NONEMPTY = 1024;
        // boosted grouped queries: boost_cut_kernel's count goes here (it runs for its transform alone: nobody reads or zeroes the word)
        static constexpr uint32_t W_BOOST_SINK = 1040;
        uint32_t *d_gout_grp = nullptr, *d_gout_n = nullptr;  // engine-owned [k] group ids and n ("the last query wins")
    } grouped;

    // Search-after paging (tkspmv_enqueue_after; after_cut_kernel, after_finish_kernel) touches no other group but the matrix either:
    // its scores go to an array of its own, the cut at the cursor rewrites that array alone, its selection runs on its own histogram,
    // candidate list and counters, and the selection kernel gets words of this group where it resets exchange state behind itself.
    // No creation stage: the first call allocates (ensure_after), 12 bytes per row; the kernels move the device words and leave them
    // zero behind every query.
    struct After {
        float *d_ay = nullptr;                  // [rows] the scores of the query in flight; -inf where a row has no entry (never written)
        unsigned long long *d_acand = nullptr;  // [rows] candidate list of the radix filter: it keeps EVERY tie at the cut
        // SelectWords; word 1024 counts the eligible rows behind the cursor (after_finish_kernel zeroes it, not the host)
        uint32_t *d_awords = nullptr;
        static constexpr uint32_t W_TOTAL = 1024;
        // engine-owned outputs of the host form ("the last query wins"): n, total | the cursor tkspmv_run_after uploads | the next cursor
        uint32_t *d_aout = nullptr;
        static constexpr uint32_t O_N = 0, O_TOTAL = 1, O_CURSOR = 4, O_NEXT = 8, N_OUT = 12;
    } after;

    // Boosted top-k (tkspmv_enqueue_boosted; boost_cut_kernel) is the search-after path with a per-row transform of the scores fused
    // into its cut: it runs on that path's scratch (ensure_after) and owns nothing but the boost tkspmv_set_boost installed.
    struct Boost {
        float *d_weight = nullptr, *d_bias = nullptr;  // [rows] each, allocated by the first tkspmv_set_boost that gives one
        bool have_weight = false, have_bias = false;   // what the installed boost consists of (neither: none is installed)
    } boost;
    // The boost of a call: query i reads weight + i * stride and bias + i * stride (either may be NULL: no multiply / no add).
    struct BoostSpec {
        const float *weight, *bias;
        size_t stride;
        const float *weight_of(int i) const { return weight ? weight + (size_t)i * stride : nullptr; }
        const float *bias_of(int i) const { return bias ? bias + (size_t)i * stride : nullptr; }
    };
    // Both of a query's arrays (where given) start at a multiple of 16 bytes: the kernels load a lane's four rows at once (NULL counts as aligned).
    static uint32_t boost_wide(const float *weight, const float *bias) {
        return ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) & 15u) == 0u ? 1u : 0u;
    }
    // Boosted range, facet and grouped queries (tkspmv_enqueue_boosted_range / _facets / _grouped; boosted_hits_kernel,
    // boosted_bins_kernel) own nothing: the first two score into the search-after path's array (ensure_after: d_ay) and read it with one
    // array kernel, the third runs boost_cut_kernel over the grouped path's array in front of that path's own launches.

    // Diagnostics: the statistics block (d_stats: setup_host_boundary; every selection counts there), the options STATS / STAMPS /
    // TRACE / WG_TIMES (setup_diagnostics), which make the engine launch the instantiations that carry the tracing and ablation
    // hooks (dbg_kernels; has_tracing_twins, elsewhere the hooks do not exist), and the full score vector of tkspmv_scores /
    // tkspmv_profile, allocated by whichever is called first.
    struct Diagnostics {
        unsigned long long *d_stats = nullptr;
        bool collect_stats = false, collect_stamps = false, dbg_kernels = false;
        unsigned long long *d_trace = nullptr;  // TKSPMV_TRACE=1: 4 launches x [grid+1][9][8] stamps
        size_t trace_words = 0;
        unsigned long long *d_wg_times = nullptr;  // option WG_TIMES: BatchParams::wg_times of the LAST batch launch (read through tkspmv_debug_trace)
        float *d_scores = nullptr;
        unsigned long long *trace_slot(uint64_t launch) const { return d_trace ? d_trace + (launch % 4) * trace_words : nullptr; }
    } diag;

    StreamParams stream_params(const float *x, int set = 0) const {
        StreamParams P{};
        const ExchangeSets::ExState &E = ex.st[set];
        P.packets = mat.packets(mat.launch_counter);
        P.pkt_row = mat.d_pkt_row;
        P.part_first = mat.d_part_first;
        P.part_count = mat.d_part_count;
        P.x = x;
        P.n_parts = (uint32_t)info.n_wave_partitions;
        P.uni_ppp = mat.uni_ppp;
        P.uni_last = mat.uni_last;
        P.cols = desc.cols;
        P.packet_bytes = pm.packet_bytes;
        P.n_sets = ex.n_sets;
        P.k = (uint32_t)desc.k;
        P.n_groups_pub = ex.n_groups_pub;
        P.gpw = ex.gpw;
        P.min_score = desc.min_score;  // converted to score units inside the kernel
        P.fixed_width = pm.fixed_width;
        P.fixed_mask = pm.fixed_width ? fixed_mask(pm.fixed_width) : 0u;
        P.gmax = E.gmax;
        P.tau_g = E.tau_g;
        P.n_reducers = grid < 8u ? grid : 8u;
        P.tau_possible = ex.groups_with_rows >= (uint32_t)desc.k ? 1u : 0u;

        P.wg_cand = E.wg_cand;
        P.ovf_cand = E.ovf;
        P.ovf_count = E.ovf_count;
        P.ovf_cap = ex.ovf_cap;
        P.scores = diag.d_scores;
        P.fused = defer.fused ? 1u : 0u;
        P.deferred = 0u;
        P.unit_inv_out = E.unit_inv;
        P.dbg = diag.collect_stats ? diag.d_stats + 4 : nullptr;
        P.stamps = diag.collect_stamps ? diag.d_stats + 16 : nullptr;
        P.trace = diag.trace_slot(mat.launch_counter);
        return P;
    }
    SelectParams select_params(uint32_t *out_idx, float *out_val, int set = 0) const {
        SelectParams S{};
        const ExchangeSets::ExState &E = ex.st[set];
        S.wg_cand = E.wg_cand;
        S.n_wg = grid;
        S.ovf_cand = E.ovf;
        S.ovf_count = E.ovf_count;
        S.ovf_cap = ex.ovf_cap;
        S.k = (uint32_t)desc.k;
        S.first_row = desc.first_row;
        S.out_scale = desc.precision == TKSPMV_Q1_7 ? (1.0f / 128.0f)
                                                    : (desc.precision == TKSPMV_FIXED ? (1.0f / 2147483648.0f) : 1.0f);  // fused tail / unit_inv_in override it
        S.unit_inv_in = nullptr;
        S.out_idx = out_idx;
        S.out_val = out_val;
        S.gmax = E.gmax;
        S.tau_g = E.tau_g;
        S.done_count = ex.d_done;
        S.n_groups_pub = ex.n_groups_pub;
        S.use_gmax = (ex.n_sets != 0u && ex.n_groups_pub >= (uint32_t)desc.k) ? 1u : 0u;
        S.stats = diag.collect_stats ? diag.d_stats : nullptr;
        S.host_out = nullptr;
        S.host_epoch = 0u;
        return S;
    }
    // The deferred single-query selection still owed, as its own small kernel.
    void settle_deferred(hipStream_t s) {
        if (!defer.pending) return;
        launch_select(defer.pending_idx, defer.pending_val, s, defer.pending_set);
        defer.pending = false;
    }
    // Every selection still owed -- to the last deferred launch, to the multi-query chains --, each as its own small kernel.
    void drain(hipStream_t s) {
        settle_deferred(s);
        drain_chain(0, s);
        if (multi.pending_group[1].n_q != 0u) {  // (only between the fork and the join of launch_multi_sequence)
            drain_chain(1, multi.side);
            (void)hipEventRecord(multi.ev_join, multi.side);
            (void)hipStreamWaitEvent(s, multi.ev_join, 0);
        }
    }
    void drain_chain(int c, hipStream_t s) {
        if (multi.pending_group[c].n_q == 0u) return;
        SelectParams S = select_params(nullptr, nullptr, 0);
        S.pos_to_row = multi.d_sell_rows;
        const MultiGroup &G = multi.pending_group[c];
        const bool serial = G.n_q > 1u && G.io[0].out_idx == G.io[1].out_idx;
        hipLaunchKernelGGL(select_group_kernel, dim3(serial ? 1u : G.n_q), dim3(SEL_THREADS), 0, s, S, set_addr(0), G, serial ? 1u : 0u);
        multi.pending_group[c].n_q = 0u;
    }
    SetAddr set_addr(int s0) const {
        SetAddr A{};
        A.gmax0 = ex.st[s0].gmax;
        A.tau_g0 = ex.st[s0].tau_g;
        A.ovf_count0 = ex.st[s0].ovf_count;
        A.wg_cand0 = ex.st[s0].wg_cand;
        A.ovf_cand0 = ex.st[s0].ovf;
        A.unit_inv0 = ex.st[s0].unit_inv;
        A.gmax_stride = ExchangeSets::GMAX_WORDS;
        A.word_stride = ExchangeSets::STATE_WORD_STRIDE;
        A.cand_stride = grid * WG_SLOTS;
        A.ovf_stride = ex.ovf_cap;
        return A;
    }
    // n <= multi_group queries in ONE launch (multi_q per pass over the matrix); their selection is owed (pending_group) to the next multi launch
    // or to drain().
    void launch_multi(const float *const *xs, uint32_t *const *out_idx, float *const *out_val, int n, hipStream_t s, int chain = 0) {
        settle_deferred(s);  // (a deferred single-query selection uses sets 0/1)
        StreamParams P = stream_params(xs[0], 0);
        P.fused = 0u;
        P.part_first = multi.d_sell_part_first;
        P.part_count = multi.d_sell_part_count;
        P.n_parts = multi.sell_parts;
        P.uni_ppp = 0u;  // (the row-per-lane stream has its own partition tables)
        P.packet_bytes = multi.sell_packet_bytes;
        P.pkt_row = nullptr;
        MultiParams M{};
        M.A = set_addr(0);
        M.part_slice0 = multi.d_sell_part_slice0;
        M.n_sel = (uint32_t)multi.multi_group;
        M.prev = multi.pending_group[chain];
        M.cur.n_q = (uint32_t)n;
        M.cur.set0 = (uint32_t)((2 * chain + multi.half[chain]) * MULTI_Q_MAX);
        for (int q = 0; q < n; ++q) {  // (one copy of the stream per PASS: the queries of a pass share it)
            BatchIO &Q = M.cur.io[q];
            Q.x = xs[q];
            Q.packets = multi.packets(mat.launch_counter + (uint64_t)(q / multi.multi_q));
            Q.out_idx = out_idx[q];
            Q.out_val = out_val[q];
        }
        mat.launch_counter += (uint64_t)((n + multi.multi_q - 1) / multi.multi_q);
        SelectParams S = select_params(nullptr, nullptr, 0);
        S.pos_to_row = multi.d_sell_rows;
        hipLaunchKernelGGL(kern.multi, dim3(grid), dim3(multi.multi_stream_waves * 64u + 64u), 0, s, P, S, M);
        multi.pending_group[chain] = M.cur;
        multi.half[chain] ^= 1;
    }
    // A sequence of queries in passes of multi_q; complete in stream order when this returns. Engines without the
    // multi-query kernel run the ordinary back-to-back sequence.
    void launch_multi_sequence(const float *const *xs, uint32_t *const *out_idx, float *const *out_val, int n, hipStream_t s) {
        if (!multi.can_multi) {
            launch_sequence(xs, out_idx, out_val, n, s);
            return;
        }
        // (two chains only with per-query result buffers: with the engine-owned pair "the last query wins" must hold)
        if (multi.multi_chains < 2 || n <= 2 * multi.multi_group || out_idx[0] == out_idx[1]) {
            for (int i = 0; i < n; i += multi.multi_group) launch_multi(xs + i, out_idx + i, out_val + i, std::min(multi.multi_group, n - i), s);
            drain(s);
            return;
        }
        drain(s);
        (void)hipEventRecord(multi.ev_fork, s);
        (void)hipStreamWaitEvent(multi.side, multi.ev_fork, 0);
        int g = 0;
        for (int i = 0; i < n; i += multi.multi_group, ++g)
            launch_multi(xs + i, out_idx + i, out_val + i, std::min(multi.multi_group, n - i), (g & 1) ? multi.side : s, g & 1);
        drain(s);  // both chains' last selections, then the caller's stream waits for the side stream
    }
    // One query, its result complete in stream order right after these launches: the stream kernel and, unless
    // fused into its tail, the select kernel.
    void launch_query(const float *x, uint32_t *out_idx, float *out_val, hipStream_t s) {
        if (desc.impl == TKSPMV_IMPL_ROW_PER_LANE && multi.can_multi) {  // the row-per-lane variant, one query per pass
            launch_multi_sequence(&x, &out_idx, &out_val, 1, s);
            return;
        }
        drain(s);
        if (radix.use_radix) {
            launch_query_radix(x, out_idx, out_val, s);
            return;
        }
        launch_stream(x, out_idx, out_val, s);
        if (!defer.fused) launch_select(out_idx, out_val, s);
    }
    // Result buffers shared by several queries (the engine-owned pair: "the last query wins"): selections run concurrently and a
    // repair writes after the fact, so only the LAST query enqueued may keep such a buffer -- query q of a launch that must not
    // write there goes to a scratch block nobody reads.
    void redirect_to_alias(BatchIO &Q, size_t q) const {
        Q.out_idx = batch.d_alias_idx + q * desc.k;
        Q.out_val = batch.d_alias_val + q * desc.k;
    }
    // The arguments of one launch of n <= BATCH_MAX queries as the engine's state stands. Changes what it must: the stream copies
    // move on by n queries (launch_counter), and the launch is counted (batch_launches: the gate's and the verdict words' turn).
    BatchArgs batch_args(const float *const *xs, uint32_t *const *out_idx, float *const *out_val, int n) {
        StreamParams P = stream_params(xs[0], 0);
        P.fused = 0u;
        P.packet_bytes = mat.batch_packet_bytes(pm);
        P.top4 = mat.compact_top4;
        SelectParams S = select_params(out_idx[0], out_val[0], 0);
        BatchParams B{};
        B.n_q = (uint32_t)n;
        B.tickets = batch.d_tickets;
        static_cast<SetAddr &>(B) = set_addr(0);
        for (int q = 0; q < n; ++q) {
            BatchIO &Q = B.io[q];
            Q.x = xs[q];
            Q.packets = mat.batch_packets(mat.launch_counter + (uint64_t)q);
            Q.out_idx = out_idx[q];
            Q.out_val = out_val[q];
            if (q + 1 < n && out_idx[q] == out_idx[n - 1]) redirect_to_alias(Q, (size_t)q);
        }
        mat.launch_counter += (uint64_t)n;
        B.n_selectors = batch.n_sel_wg;
        B.local = local.use_local;
        B.pace_quads = local.pace_quads;
        B.pace_levels = local.pace_levels;
        B.pace_base = local.pace_base;
        B.pace_period = outlasts_timetable(local.pace_period_ns, n) ? 0u : period_units(local.pace_period_ns);
        B.pace_adapt = local.pace_adapt_on ? local.d_pace_adapt : nullptr;
        B.wg_pace = local.pace_carry ? local.d_wg_pace : nullptr;
        B.wg_times = diag.d_wg_times;
        B.prior_block = reinterpret_cast<uint32_t *>(local.d_wg_prior + grid);
        B.gate_parity = (uint32_t)(batch.batch_launches & 1u);
        // (four words: a launch zeroes the word of the launch after the next)
        B.verdict = trust.d_verdict + 16 * (batch.batch_launches & 3u);
        B.verdict_next = trust.d_verdict + 16 * ((batch.batch_launches + 2u) & 3u);
        ++batch.batch_launches;
        if (local.use_local) {
            B.wg_prior = local.d_wg_prior;
            B.wg_sig = local.d_wg_sig;
            B.local_beta = local.local_beta;
        }
        B.lslots = batch.d_rec_slots;
        B.lused = batch.d_rec_used;
        B.lslots_stride = grid * WG_SLOTS;
        B.lused_stride = grid;
        B.ovf_epoch = ex.d_ovf_epoch;
        B.ovf_lists = std::min(ex.ovf_lists, 4u);  // (engines with one list per set -- the multi-query ones -- lend the batch kernel their first four)
        return BatchArgs{P, S, B};
    }
    // n <= BATCH_MAX queries in one launch of the batch kernel; results complete in stream order after the launch(es). With
    // local thresholds: the kernel of the checked local thresholds, then the exact kernel for whatever failed its check (that
    // launch is empty -- every workgroup reads the verdict word and leaves -- unless a query was unlike the ones before it). A
    // launch the host can watch (trust.has_room, the engine's own stream) leaves its verdict in the host's ring too, and while the
    // host trusts, the exact kernel stays away: settle() repairs.
    void launch_batch(const float *const *xs, uint32_t *const *out_idx, float *const *out_val, int n, hipStream_t s) {
        // (first: the region's start event goes with this kernel, if one is waiting; last: the stop event, if this is the region's final launch)
        auto go = [&](batch_fn fn, const BatchArgs &args, bool last) {
            hipEvent_t a = batch.ext_start, b = (last && batch.ext_last) ? batch.ext_stop : nullptr;
            batch.ext_start = nullptr;
            if (b) batch.ext_stop = nullptr;
            if (batch.ext_record) {
                if (a) (void)hipEventRecord(a, s);
                hipLaunchKernelGGL(fn, dim3(grid), dim3(block + 64), 0, s, args);
                if (b) (void)hipEventRecord(b, s);
            } else if (a || b) {
                hipExtLaunchKernelGGL(fn, dim3(grid), dim3(block + 64), 0, s, a, b, 0, args);
            } else {
                hipLaunchKernelGGL(fn, dim3(grid), dim3(block + 64), 0, s, args);
            }
        };
        drain(s);
        BatchArgs A = batch_args(xs, out_idx, out_val, n);
        const bool watched = local.use_local && s == stream && trust.has_room();
        const bool trusted = watched && trust.trusts();
        uint32_t slot = 0u;
        if (watched) {
            slot = (uint32_t)(trust.verdict_seq++ % Trust::VERDICT_RING);
            trust.h_verdict[slot] = 0ull;
            A.B.verdict_host = trust.h_verdict_dev + slot;
        }
        if (local.use_local) go(kern.batch[1], A, trusted);
        if (!trusted) {
            BatchArgs R = A;
            R.B.repair = local.use_local ? 1u : 0u;
            go(kern.batch[0], R, true);
        }
        if (!watched) return;
        if (trusted) ++trust.trusted_launches;
        else if (trust.distrust_left != 0u) --trust.distrust_left;
        trust.pending_checks.push_back(Trust::PendingCheck{A, slot, trusted});
    }
    // The host has just waited for the engine's stream: look at the verdicts of the launches enqueued since it last did. A flagged
    // query of a TRUSTED launch (no repair launch behind it) is repaired now -- exact launch of the flagged queries, one more wait --;
    // any failure brings the in-stream repair launch back for a while. Returns hipSuccess, or the error of the repair's wait.
    hipError_t settle() {
        bool late = false;
        const size_t n_pending = trust.pending_checks.size();
        for (size_t i = 0; i < n_pending; ++i) {
            Trust::PendingCheck &pc = trust.pending_checks[i];
            const unsigned long long v = const_cast<volatile unsigned long long *>(trust.h_verdict)[pc.slot];
            const uint32_t mask = (uint32_t)(v >> 32);
            // (a word that is not complete: the launch was not waited for after all -- a caller polling an event of its own; such a
            //  launch counts as a failure of trust, not of a check: everything of it is run again below if nobody repaired it)
            const bool complete = (uint32_t)v == pc.A.B.n_q;
            if (complete && mask == 0u) {
                if (trust.clean_seen != 0xFFFFFFFFu) ++trust.clean_seen;
                continue;
            }
            trust.clean_seen = 0u;
            trust.distrust_left = Trust::DISTRUST_LAUNCHES;
            if (!pc.trusted) continue;  // (its in-stream repair launch has dealt with it)
            BatchArgs R = pc.A;
            R.B.repair = 2u;
            R.B.repair_mask = complete ? mask : (R.B.n_q >= 32u ? 0xFFFFFFFFu : ((1u << R.B.n_q) - 1u));
            R.B.verdict_host = nullptr;
            // (a launch that was not the last one enqueued must not write the engine-owned pair again after the fact)
            if (i + 1u < n_pending)
                for (uint32_t q = 0; q < R.B.n_q; ++q)
                    if (R.B.io[q].out_idx == host.d_out_idx) redirect_to_alias(R.B.io[q], q);
            hipLaunchKernelGGL(kern.batch[0], dim3(grid), dim3(block + 64), 0, stream, R);
            ++trust.late_repairs;
            late = true;
        }
        trust.pending_checks.clear();
        return late ? hipStreamSynchronize(stream) : hipSuccess;
    }
    // The host waits for the engine's stream, then looks at the verdicts (settle).
    int wait_idle(std::string &err) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(settle());
        return TKSPMV_OK;
    }
    // The time of `region` -- launches on the engine's stream -- by the events ev0 and ev1 recorded around it; the host waits for ev1.
    template <class Region>
    int bracket_ms(float &ms, std::string &err, Region region) {
        HIP_TRY(hipEventRecord(ev0, stream));
        region();
        HIP_TRY(hipEventRecord(ev1, stream));
        HIP_TRY(hipEventSynchronize(ev1));
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        return TKSPMV_OK;
    }
    // A back-to-back sequence of queries given as pointer lists: batch kernel launches of up to batch_max queries
    // when it is available, else deferred selection.
    void launch_sequence(const float *const *xs, uint32_t *const *out_idx, float *const *out_val, int n, hipStream_t s) {
        if (!batch.can_batch) {
            for (int i = 0; i < n; ++i) launch_deferred(xs[i], out_idx[i], out_val[i], s);
            drain(s);
            return;
        }
        for (int i = 0; i < n; i += batch.batch_max) {
            batch.ext_last = i + batch.batch_max >= n;
            launch_batch(xs + i, out_idx + i, out_val + i, std::min(batch.batch_max, n - i), s);
        }
    }
    // One query of a back-to-back sequence: its selection runs inside the NEXT deferred launch (or in drain()).
    void launch_deferred(const float *x, uint32_t *out_idx, float *out_val, hipStream_t s, const FilterParams *F = nullptr) {
        if (!defer.can_defer) {
            launch_query(x, out_idx, out_val, s);
            return;
        }
        StreamParams P = stream_params(x, defer.cur_set);
        P.fused = 0u;
        P.deferred = 1u;
        SelectParams S{};  // n_wg = 0: nothing owed
        if (defer.pending) {
            S = select_params(defer.pending_idx, defer.pending_val, defer.pending_set);
            S.unit_inv_in = ex.st[defer.pending_set].unit_inv;
        }
        ++mat.launch_counter;
        launch_stream_kernel(false, F, s, P, S);
        defer.pending = true;
        defer.pending_set = defer.cur_set;
        defer.pending_idx = out_idx;
        defer.pending_val = out_val;
        defer.cur_set ^= 1;
    }
    // One launch of the streaming kernel: stream_kernel, or stream_filter_kernel with the allow-mask F.
    void launch_stream_kernel(bool scores, const FilterParams *F, hipStream_t s, const StreamParams &P, const SelectParams &S) const {
        if (F) hipLaunchKernelGGL(kern.filter[scores], dim3(grid), dim3(block + 64), 0, s, P, S, *F);
        else hipLaunchKernelGGL(kern.stream[scores], dim3(grid), dim3(block + 64), 0, s, P, S);
    }
    // What launch_range, launch_facets and launch_match share: n queries in launches of at most max_q, each one scan of the matrix. R is
    // RangeParams, FacetParams or MatchParams, used by field name: the stream copies, the masks' geometry and each launch's q0 / n_q are
    // filled here; chunk(i, c) points the rest at the queries [i, i + c). Zeroing the outputs in front stays with the caller.
    template <class Params, class Fn, class Chunk>
    void launch_scan(Params &R, Fn fn, const StreamParams &P, int n, int max_q, size_t mask_stride, hipStream_t s, Chunk chunk) const {
        R.n_replicas = mat.d_replicas.empty() ? 1u : (uint32_t)std::min<size_t>(mat.d_replicas.size(), 16);
        for (uint32_t r = 0; r < R.n_replicas; ++r) R.replicas[r] = mat.packets(r);
        R.mask_stride = (uint32_t)mask_stride;
        R.mask_words = mask_words();
        for (int i = 0; i < n; i += max_q) {
            const int c = std::min(max_q, n - i);
            R.q0 = (uint32_t)i;
            R.n_q = (uint32_t)c;
            chunk(i, c);
            hipLaunchKernelGGL(fn, dim3(grid), dim3(512), 0, s, P, R);
        }
    }
    // The period of a scan launch of c queries that keep a timetable (range and facets; option RANGE_PERIOD): the timetable of
    // launch_batch; one partition per wave, or no timetable.
    uint32_t scan_period(int c, const StreamParams &P) const {
        const uint32_t period_ns = range.range_period_set ? range.range_period_ns : local.pace_period_ns;
        return (outlasts_timetable(period_ns, c) || (uint64_t)P.n_parts > (uint64_t)grid * 8u) ? 0u : period_units(period_ns);
    }
    // n range queries (query i: x = xs + i * cols, threshold thresholds[i], mask = mask + i * stride words or none), complete in
    // stream order when this returns: the counters are zeroed in front, then launches of up to RANGE_MAX queries. No engine state is
    // read or written besides the matrix: the stream copies rotate with the query's number in THIS call.
    void launch_range(const float *xs, int n, const float *thresholds, const uint32_t *mask, size_t stride, uint32_t *idx, float *val,
                      uint32_t capacity, uint32_t *counts, hipStream_t s) const {
        (void)hipMemsetAsync(counts, 0, (size_t)n * 4, s);
        const StreamParams P = stream_params(xs);
        RangeParams R{};
        R.capacity = capacity;
        R.first_row = desc.first_row;
        launch_scan(R, kern.range[mask != nullptr], P, n, Range::RANGE_MAX, stride, s, [&](int i, int c) {
            R.xs = xs + (size_t)i * desc.cols;
            R.thresholds = thresholds + i;
            R.mask = mask ? mask + (size_t)i * stride : nullptr;
            R.counts = counts + i;
            R.idx = idx ? idx + (size_t)i * capacity : nullptr;
            R.val = val ? val + (size_t)i * capacity : nullptr;
            R.period = scan_period(c, P);
        });
    }
    // n facet queries (launch_range's queries; bin of local row r: labels[r], none when that is >= n_bins), complete in stream order
    // when this returns: counts, best and totals are zeroed in front, then launches of up to RANGE_MAX queries whose kernels add to
    // counts / totals and raise best to the maximum of (order key << 32 | global row), then one closing launch that turns the non-zero
    // maxima into {row, score bits}. No engine state is read or written besides the matrix.
    void launch_facets(const float *xs, int n, const float *thresholds, const uint32_t *mask, size_t stride, const uint32_t *labels, uint32_t n_bins,
                       uint32_t *counts, tkspmv_facet_best *best, uint32_t *totals, hipStream_t s) const {
        const size_t n_out = (size_t)n * n_bins;
        if (n_out) (void)hipMemsetAsync(counts, 0, n_out * 4, s);
        if (best && n_out) (void)hipMemsetAsync(best, 0, n_out * 8, s);
        if (totals) (void)hipMemsetAsync(totals, 0, (size_t)n * 4, s);
        const StreamParams P = stream_params(xs);
        FacetParams R{};
        R.labels = labels;
        R.n_bins = n_bins;
        R.lds_bins = n_bins <= range.facet_lds_bins ? range.facet_lds_bins : 0u;
        R.first_row = desc.first_row;
        R.args_tag = FACET_ARGS_TAG;
        launch_scan(R, kern.facet[mask != nullptr], P, n, Range::RANGE_MAX, stride, s, [&](int i, int c) {
            R.xs = xs + (size_t)i * desc.cols;
            R.thresholds = thresholds + i;
            R.mask = mask ? mask + (size_t)i * stride : nullptr;
            R.counts = counts + (size_t)i * n_bins;
            R.best = best ? reinterpret_cast<unsigned long long *>(best) + (size_t)i * n_bins : nullptr;
            R.totals = totals ? totals + i : nullptr;
            R.period = scan_period(c, P);
        });
        if (best && n_out) {
            const uint32_t cgrid = (uint32_t)std::min<size_t>((n_out + 255u) / 256u, 16384u);
            hipLaunchKernelGGL(facet_close_kernel, dim3(cgrid), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(best), (unsigned long long)n_out);
        }
    }
    // Why term predicates are not served by this engine (nullptr: they are; with_mask: the call carries an allow-mask). Like row
    // vectors, and unlike filtered queries, the approximate per-partition engines are served: which columns a row has does not depend
    // on how rows are selected.
    const char *match_unsupported(bool with_mask) const {
        if (!kern.match[0]) return "term predicates need an fp32 packet stream (TKSPMV_F32)";
        if (pm.n_packets != 0u && (!mat.d_packets || !mat.d_pkt_row || !mat.d_part_first)) return "term predicates are read from the wave-BSCSR packets: this engine does not hold them";
        return with_mask ? filter_unsupported() : nullptr;
    }
    // n term predicates (query i: table = clauses + i * cstride words, predicate preds[i], mask = mask + i * mstride words or none;
    // result at out + i * ostride words, count at counts[i] or none), complete in stream order when this returns: the outputs are
    // zeroed in front -- the masks' own words only --, then launches of up to MATCH_MAX queries. No engine state is read or written
    // besides the matrix: the stream copies rotate with the query's number in THIS call.
    void launch_match(const uint32_t *clauses, size_t cstride, const tkspmv_match *preds, int n, const uint32_t *mask, size_t mstride, uint32_t *out,
                      size_t ostride, uint32_t *counts, hipStream_t s) const {
        const size_t words = mask_words();
        if (n == 1 || ostride == words) (void)hipMemsetAsync(out, 0, (size_t)n * words * 4, s);
        else (void)hipMemset2DAsync(out, ostride * 4, 0, words * 4, (size_t)n, s);
        if (counts) (void)hipMemsetAsync(counts, 0, (size_t)n * 4, s);
        MatchParams R{};
        R.clause_stride = cstride;
        R.out_stride = ostride;
        R.args_tag = MATCH_ARGS_TAG;
        // (no query vector and no timetable: MatchParams has neither xs nor period)
        launch_scan(R, kern.match[mask != nullptr], stream_params(nullptr), n, Match::MATCH_MAX, mstride, s, [&](int i, int) {
            R.clauses = clauses + (size_t)i * cstride;
            R.preds = preds + i;
            R.mask = mask ? mask + (size_t)i * mstride : nullptr;
            R.out = out + (size_t)i * ostride;
            R.counts = counts ? counts + i : nullptr;
        });
    }
    // Why stored rows cannot be expanded by this engine (nullptr: they can). Unlike filtered queries, the approximate per-partition
    // engines are served: extraction does not depend on how rows are selected.
    const char *row_vectors_unsupported() const {
        if (!kern.row_vectors) return "row vectors need an fp32 packet stream (TKSPMV_F32)";
        if (pm.n_packets != 0u && (!mat.d_packets || !mat.d_pkt_row || !mat.d_part_first)) return "row vectors are read from the wave-BSCSR packets: this engine does not hold them";
        return nullptr;
    }
    // The matrix as the kernels that locate stored rows see it: what RowVecParams and ScoreRowsParams share, set by field name.
    template <class Params>
    void fill_row_view(Params &R) const {
        R.packets = mat.d_packets;
        R.pkt_row = mat.d_pkt_row;
        R.part_first = mat.d_part_first;
        R.part_count = mat.d_part_count;
        R.n_packets = pm.n_packets;
        R.n_parts = (uint32_t)pm.part_first.size();
        R.packet_bytes = pm.packet_bytes;
        R.cols = desc.cols;
        R.rows = desc.rows;
        R.first_row = desc.first_row;
    }
    // Rows ids[0 .. n) as dense vectors xs[n][cols] (len[n]: their entries, optional), complete in stream order when this returns:
    // one wave per row. Stream copy 0 is read whatever stream_replicas says.
    void launch_row_vectors(const uint32_t *ids, int n, float *xs, uint32_t *len, hipStream_t s) const {
        RowVecParams R{};
        fill_row_view(R);
        R.ids = ids;
        R.xs = xs;
        R.len = len;
        hipLaunchKernelGGL(kern.row_vectors, dim3((uint32_t)n), dim3(64), 0, s, R);
    }
    // Scores of the rows ids + q * stride [0 .. n_rows) for the queries xs[q], q < n_q, into scores[n_q][n_rows], complete in stream
    // order when this returns. A wave per list entry and chunk of queries: with one list for every query (stride = 0) the queries are
    // cut into just as many chunks as it takes to fill the device, so that a row is located as few times as possible. The grid's y
    // counts the chunks: more of them than a grid has go into further launches. Stream copy 0 is read whatever stream_replicas says.
    void launch_score_rows(const float *xs, int n_q, const uint32_t *ids, int n_rows, size_t stride, float *scores, hipStream_t s) const {
        ScoreRowsParams R{};
        fill_row_view(R);
        R.ids_stride = stride;
        R.n_rows = (uint32_t)n_rows;
        const uint32_t wgs_full = std::max(1u, info.num_cus) * 8u;  // workgroups of 4 waves that fill the device
        const uint32_t wgs_rows = (uint32_t)(((uint64_t)n_rows + SCORE_ROWS_WAVES - 1u) / SCORE_ROWS_WAVES);
        const uint32_t chunks = stride != 0u ? (uint32_t)n_q : std::min<uint32_t>((uint32_t)n_q, std::max(1u, wgs_full / wgs_rows));
        R.q_per_item = ((uint32_t)n_q + chunks - 1u) / chunks;
        constexpr uint32_t GRID_Y = 65535u;
        for (uint64_t q = 0; q < (uint64_t)n_q; q += (uint64_t)GRID_Y * R.q_per_item) {
            R.n_q = (uint32_t)std::min<uint64_t>((uint64_t)n_q - q, (uint64_t)GRID_Y * R.q_per_item);
            R.xs = xs + q * desc.cols;
            R.ids = ids + q * stride;
            R.scores = scores + q * (uint64_t)n_rows;
            hipLaunchKernelGGL(kern.score_rows, dim3(wgs_rows, (R.n_q + R.q_per_item - 1u) / R.q_per_item), dim3(64u * SCORE_ROWS_WAVES), 0, s, R);
        }
    }
    // One statistic of every local row into out[0 .. rows), complete in stream order when this returns: out is zeroed in front (rows
    // without entries are never written by the kernel), then one pass over stream copy 0 with the scan kernels' geometry. No engine
    // state is read or written besides the matrix.
    void launch_row_stats(int kind, float *out, hipStream_t s) const {
        if (desc.rows == 0u) return;
        (void)hipMemsetAsync(out, 0, (size_t)desc.rows * 4, s);
        if (pm.n_packets == 0u) return;
        const RowStatsParams R{mat.d_packets, out, desc.rows};
        hipLaunchKernelGGL(kern.row_stats[kind], dim3(grid), dim3(512), 0, s, stream_params(nullptr), R);
    }
    // Vectors one assign_kernel launch serves: as many as fit the kernel's 64 KiB of LDS at the engine's column tier (16 / 4 / 1).
    int assign_pass() const { return assign_vectors_per_pass(fmt.xcols); }
    // Labels and best scores of every local row for the vectors xs[0 .. n), which are the vectors q_base .. q_base + n of their call,
    // complete in stream order when this returns. q_base = 0: both outputs are zeroed in front (rows without entries are never written
    // by the kernel) and the first launch stores unconditionally; every later launch -- of this call or, q_base != 0, of the call's
    // later chunks -- merges with the stored pair and needs best. No engine state is read or written besides the matrix.
    void launch_assign(const float *xs, int n, uint32_t q_base, uint32_t *labels, float *best, hipStream_t s) const {
        if (desc.rows == 0u) return;
        if (q_base == 0u) {
            (void)hipMemsetAsync(labels, 0, (size_t)desc.rows * 4, s);
            if (best) (void)hipMemsetAsync(best, 0, (size_t)desc.rows * 4, s);
        }
        launch_assign_passes(kern.assign, xs, n, q_base, s, [&](const float *x, uint32_t n_q, uint32_t q0) { return AssignParams{mat.d_packets, x, labels, best, desc.rows, n_q, q0}; });
    }
    // The n best of the call's `total` vectors for every local row, in order, for the vectors xs[0 .. cnt), which are the vectors
    // q_base .. q_base + cnt of their call, complete in stream order when this returns. q_base = 0: nearest_fill_kernel writes every
    // row's default list in front (what the two memsets are to launch_assign: rows without entries and rows outside the mask are never
    // written by the streaming kernel) and the first launch stores its lists as they are; every later launch -- of this call or,
    // q_base != 0, of the call's later chunks -- merges with the stored list. No engine state is read or written besides the matrix.
    void launch_nearest(const float *xs, int cnt, uint32_t q_base, uint32_t total, uint32_t n, const uint32_t *mask, uint32_t *labels, float *scores,
                        hipStream_t s) const {
        if (desc.rows == 0u) return;
        if (q_base == 0u) {
            const uint64_t words = (uint64_t)desc.rows * n;
            const uint32_t fill_grid = (uint32_t)std::min<uint64_t>((words + 255u) / 256u, (uint64_t)std::max(1u, info.num_cus) * 32u);
            hipLaunchKernelGGL(nearest_fill_kernel, dim3(fill_grid), dim3(256), 0, s, mask, labels, scores, desc.rows, n, total);
        }
        launch_assign_passes(kern.nearest[(n > 1u) + (n > 2u)], xs, cnt, q_base, s,
                             [&](const float *x, uint32_t n_q, uint32_t q0) { return NearestParams{mat.d_packets, x, mask, labels, scores, desc.rows, n, n_q, q0}; });
    }
    // The passes of launch_assign and launch_nearest behind their zeroing: one launch of fn over stream copy 0 per assign_pass() vectors,
    // with the scan kernels' geometry; params(x, n_q, q0) are the AssignParams / NearestParams of the pass of n_q vectors at x, which are
    // the call's vectors q0 .. q0 + n_q. Not a launch_scan call: neither struct has a stream-copy table or mask geometry to fill, the
    // chunk size is the format's, and q0 continues across the host forms' chunks (q_base), which launch_scan restarts at 0 per call.
    template <class Fn, class MakeParams>
    void launch_assign_passes(Fn fn, const float *xs, int n, uint32_t q_base, hipStream_t s, MakeParams params) const {
        if (pm.n_packets == 0u) return;
        const StreamParams P = stream_params(nullptr);
        const int qp = assign_pass();
        for (int i = 0; i < n; i += qp)
            hipLaunchKernelGGL(fn, dim3(grid), dim3(512), 0, s, P, params(xs + (size_t)i * desc.cols, (uint32_t)std::min(qp, n - i), q_base + (uint32_t)i));
    }
    // Why column statistics are not served by this engine (nullptr: they are; with_mask: the call carries an allow-mask). Served where
    // row statistics are; among the rows of a mask, where filtered queries are (match_unsupported's rule).
    const char *col_stats_unsupported(bool with_mask) const {
        if (const char *why = row_vectors_unsupported()) return why;
        return with_mask ? filter_unsupported() : nullptr;
    }
    // One statistic of every column over n sets of rows (set i: the rows of mask + i * mstride words, or all rows without a mask; result
    // at out + i * ostride words, cols of them), complete in stream order when this returns: the outputs are zeroed in front -- the sets'
    // own words only --, then launches of up to COL_STATS_MAX sets whose workgroups add to / raise the words, then for MAX / MIN one
    // closing launch that turns order keys into floats. No engine state is read or written besides the matrix: the stream copies
    // rotate with the set's number in THIS call.
    void launch_col_stats(int kind, int n, const uint32_t *mask, size_t mstride, uint32_t *out, size_t ostride, hipStream_t s) const {
        const size_t cols = desc.cols;
        if (cols == 0u) return;
        if (n == 1 || ostride == cols) (void)hipMemsetAsync(out, 0, (size_t)n * cols * 4, s);
        else (void)hipMemset2DAsync(out, ostride * 4, 0, cols * 4, (size_t)n, s);
        const bool ext = kind != TKSPMV_COL_NNZ;
        const uint32_t negate = kind == TKSPMV_COL_MIN ? 0x80000000u : 0u;
        if (pm.n_packets != 0u) {
            ColStatsParams R{};
            R.out_stride = ostride;
            R.negate = negate;
            R.args_tag = COL_STATS_ARGS_TAG;
            launch_scan(R, kern.col_stats[ext][mask != nullptr], stream_params(nullptr), n, ColStats::COL_STATS_MAX, mstride, s, [&](int i, int) {
                R.mask = mask ? mask + (size_t)i * mstride : nullptr;
                R.out = out + (size_t)i * ostride;
            });
        }
        if (ext) {
            const uint32_t cgrid = (uint32_t)std::min<size_t>(((size_t)n * cols + 255u) / 256u, 16384u);
            hipLaunchKernelGGL(col_stats_close_kernel, dim3(cgrid), dim3(256), 0, s, out, (uint64_t)ostride, (uint32_t)cols, (uint32_t)n, negate);
        }
    }
    // Which sink a label-sums call takes when its flags force none: the LDS sink where the tier has one (1024 and 4096 columns) and
    // the bins need at most LABEL_SUMS_LDS_MAX_WINDOWS launches, the direct sink otherwise. The crossover is measured, not reasoned:
    // profiles/label_sums_probe.json (1M x 1024, 20 entries per row, B = 8 bins per launch) has the two sinks side by side. A launch
    // of the LDS sink costs 42 .. 65 us whatever its window; the direct sink 0.93 .. 1.3 ms for 8 bins and more (2.7 ms for one bin:
    // every atomic of a column meets in one word). The LDS sink wins at 128 bins (16 launches: 806 us against 983), the direct sink
    // at 256 (32 launches: 1348 against 932): the rule changes sides between those two measured points. DESIGN.md section 3.23 has
    // the table.
    static constexpr uint32_t LABEL_SUMS_LDS_MAX_WINDOWS = 16;
    bool label_sums_lds_sink(uint32_t n_bins) const {
        const uint32_t B = label_sums_lds_bins(fmt.xcols);
        return kern.label_sums[1] != nullptr && B != 0u && (n_bins + B - 1u) / B <= LABEL_SUMS_LDS_MAX_WINDOWS;
    }
    // The int64 sums of every bin and column (labels[r]: the bin of local row r, none when >= n_bins) into sums[n_bins][cols], complete
    // in stream order when this returns: sums is zeroed in front unless the call accumulates, then one launch of the direct sink, or one
    // launch of the LDS sink per window of 8192 / tier bins, over stream copy 0 with the scan kernels' geometry. No engine state is read
    // or written besides the matrix.
    void launch_label_sums(const uint32_t *labels, uint32_t n_bins, int32_t quantum_exp, bool accumulate, bool lds, int64_t *sums, hipStream_t s) const {
        const size_t words = (size_t)n_bins * desc.cols;
        if (words == 0u) return;
        if (!accumulate) (void)hipMemsetAsync(sums, 0, words * 8, s);
        if (desc.rows == 0u || pm.n_packets == 0u) return;
        const StreamParams P = stream_params(nullptr);
        LabelSumsParams R{mat.d_packets, labels, reinterpret_cast<unsigned long long *>(sums), desc.rows, n_bins, 0u, quantum_exp};
        if (!lds) {
            hipLaunchKernelGGL(kern.label_sums[0], dim3(grid), dim3(512), 0, s, P, R);
            return;
        }
        for (uint32_t b0 = 0; b0 < n_bins; b0 += label_sums_lds_bins(fmt.xcols)) {
            R.b0 = b0;
            hipLaunchKernelGGL(kern.label_sums[1], dim3(grid), dim3(512), 0, s, P, R);
        }
    }
    // sums[n_bins][cols] as floats into out (TKSPMV_SUMS_FLOAT) or as unit vectors (TKSPMV_SUMS_UNIT: a bin whose norm is 0 or
    // overflows is not written), complete in stream order when this returns: one workgroup of 64 threads per bin.
    void launch_sums_close(const int64_t *sums, uint32_t n_bins, int32_t quantum_exp, int mode, float *out, hipStream_t s) const {
        if (n_bins == 0u || desc.cols == 0u) return;
        hipLaunchKernelGGL(label_sums_close_kernel, dim3(n_bins), dim3(64), 0, s, reinterpret_cast<const long long *>(sums), out, (uint32_t)desc.cols, quantum_exp,
                           mode == TKSPMV_SUMS_UNIT ? 1u : 0u);
    }
    // Why filtered queries are not served by this engine (nullptr: they are).
    const char *filter_unsupported() const {
        if (!is_fp32(fmt)) return "filtered queries need fp32 values (TKSPMV_F32)";
        if (!kern.filter[0]) return "filtered queries need an fp32 packet stream";
        if (radix.approx_parts) return "filtered queries are exact only: partitions > 1 with k > k_per_partition is the approximate per-partition path";
        if (!mat.d_packets || !mat.d_pkt_row) return "filtered queries stream the wave-BSCSR packets: this engine does not hold them";
        return nullptr;
    }
    bool range_unsupported(std::string &err) const {  // (fills err)
        const char *why = filter_unsupported();
        if (why) err = std::string("range queries share the filtered path's scope: ") + why;
        return why != nullptr;
    }
    // A sequence of filtered queries (query i: x = xs[i], mask = mask + i * stride words), complete in stream order when this
    // returns. The launch scheme is the one of a single exact query: deferred selections where the engine has them, else stream +
    // select, scores + radix select where the engine takes that path. Never the batch, single or multi-query kernels: their carried
    // thresholds assume the score distribution of the query before, which a per-query filter breaks.
    void launch_filtered(const float *const *xs, const uint32_t *mask, size_t stride, uint32_t *const *out_idx, float *const *out_val, int n,
                         hipStream_t s) {
        drain(s);  // (a deferred selection still owed uses the same exchange-state sets)
        for (int i = 0; i < n; ++i) {
            const FilterParams F{mask + (size_t)i * stride, mask_words()};
            if (radix.use_radix) {
                launch_query_radix(xs[i], out_idx[i], out_val[i], s, &F);
            } else if (defer.can_defer) {
                launch_deferred(xs[i], out_idx[i], out_val[i], s, &F);
            } else {
                launch_stream(xs[i], out_idx[i], out_val[i], s, false, &F);
                if (!defer.fused) launch_select(out_idx[i], out_val[i], s);
            }
        }
        drain(s);
    }
    // Why grouped queries are not served by this engine (nullptr: they are; with_mask: the call carries an allow-mask).
    const char *grouped_unsupported(bool with_mask) const {
        if (radix.approx_parts) return "grouped queries are exact only: partitions > 1 with k > k_per_partition is the approximate per-partition path";
        if (!mat.d_packets || !mat.d_pkt_row) return "grouped queries stream the wave-BSCSR packets: this engine does not hold them";
        return with_mask ? filter_unsupported() : nullptr;
    }
    // The array select -- scores in an array, four radix_hist_kernel passes, radix_filter_kernel, select_kernel -- as launch_grouped,
    // launch_after and launch_query_radix share it. order_key: the host twin of the device function (kernels/common.hpp).
    static uint32_t order_key(float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    // The radix select of scores[n] on a path's own words (SelectWords) and candidate list of `cap` entries ...
    static RadixParams radix_params(const float *scores, uint32_t n, uint32_t k, uint32_t kmin, uint32_t *words, unsigned long long *cand, uint32_t cap) {
        return RadixParams{scores, n, k, kmin, /*hist*/ words, /*ovf_cand*/ cand, /*ovf_count*/ words + SelectWords::W_COUNT, /*ovf_cap*/ cap};
    }
    // ... and the selection kernel behind it: no slots, no published maxima, every candidate comes from the list, as an index into
    // the array (the caller sets pos_to_row where that is not a local row, and the outputs per query).
    SelectParams array_select_params(uint32_t *words, unsigned long long *cand, uint32_t cap) const {
        SelectParams S{};
        S.wg_cand = cand;  // (n_wg = 0: the selection still forms the address of slot 0)
        S.ovf_cand = cand;
        S.ovf_count = words + SelectWords::W_COUNT;
        S.ovf_cap = cap;
        S.k = (uint32_t)desc.k;
        S.first_row = desc.first_row;
        S.out_scale = 1.0f;  // the scores kernel already wrote final scores
        S.tau_g = words + SelectWords::W_TAU;
        S.done_count = words + SelectWords::W_DONE;
        return S;
    }
    // The four histogram passes and the filter pass over R's n scores. The caller has zeroed the histogram in front.
    static void launch_radix_passes(const RadixParams &R, uint32_t n, hipStream_t s) {
        const uint32_t rgrid = std::max(1u, std::min(256u, (n + RADIX_THREADS * 4u - 1u) / (RADIX_THREADS * 4u)));
        for (int pass = 0; pass < 4; ++pass) hipLaunchKernelGGL(radix_hist_kernel, dim3(rgrid), dim3(RADIX_THREADS), 0, s, R, pass);
        hipLaunchKernelGGL(radix_filter_kernel, dim3(rgrid), dim3(RADIX_THREADS), 0, s, R);
    }
    // The grid of a kernel whose lanes take lane_rows rows each: enough workgroups of `threads` for `rows`, at most 8 per CU.
    uint32_t rows_grid(uint32_t rows, uint32_t threads, uint32_t lane_rows) const {
        return std::max(1u, std::min(std::max(1u, info.num_cus) * 8u, (uint32_t)(((uint64_t)rows + threads * lane_rows - 1u) / (threads * lane_rows))));
    }
    // A [rows] score array of a path's own, recorded: -inf where a row has no entry (the scores kernel never writes there).
    hipError_t alloc_ninf_scores(float *&p) {
        const std::vector<float> ninf(std::max<size_t>(desc.rows, 1), -std::numeric_limits<float>::infinity());
        float *y = nullptr;
        hipError_t e = alloc(y, ninf.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(y, ninf.data(), ninf.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) p = y;  // (*p stays NULL until the array is filled)
        return e;
    }
    // A sequence of grouped queries (query i: x = xs + i * cols, mask = mask + i * stride words or none; results at out_* + i *
    // out_stride, the number of real entries at out_n + i * n_stride), complete in stream order when this returns: per query the SpMV-only kernel, the reduction to groups, the radix
    // select over the groups and the selection kernel ranking the groups' representatives. No exchange set, record, verdict, carried
    // threshold or deferred selection is read or written: the SpMV-only kernels touch none, and the selection kernel is given this
    // path's own words. Only mat.launch_counter moves.
    // With a boost (tkspmv_enqueue_boosted_grouped) boost_cut_kernel runs behind the SpMV-only kernel, from the top (no cursor): it
    // writes the transformed scores in place, and everything behind it reads them. Its count goes to a word of this path nobody reads.
    void launch_grouped(const float *xs, int n, const uint32_t *mask, size_t stride, uint32_t *out_idx, float *out_val, uint32_t *out_grp,
                        size_t out_stride, uint32_t *out_n, size_t n_stride, hipStream_t s, const BoostSpec *boost = nullptr) {
        using namespace grouped_kernels;
        const Grouped &Q = grouped;
        GroupParams G{};
        G.scores = Q.d_gy;
        G.groups = Q.d_groups;
        G.gkey = Q.d_gkey;
        G.gscore = Q.d_gscore;
        G.grow = Q.d_grow;
        G.n_nonempty = Q.d_gwords + Grouped::W_NONEMPTY;
        G.rows = desc.rows;
        G.n_groups = Q.n_groups;
        G.kmin = order_key(desc.min_score);
        const RadixParams R = radix_params(Q.d_gscore, Q.n_groups, (uint32_t)desc.k, G.kmin, Q.d_gwords, Q.d_gcand, Q.n_groups);
        SelectParams S = array_select_params(Q.d_gwords, Q.d_gcand, Q.n_groups);  // (a candidate is a group's index ...
        S.pos_to_row = Q.d_grow;                                                   //  ... and stands for its representative's row)
        GroupIdsParams I{};
        I.groups = Q.d_groups;
        I.n_nonempty = G.n_nonempty;
        I.k = (uint32_t)desc.k;
        I.rows = desc.rows;
        I.first_row = desc.first_row;
        const uint32_t best_grid = rows_grid(desc.rows, GROUP_THREADS, GROUP_LANE_ROWS);
        const uint32_t split_grid = (Q.n_groups + GROUP_THREADS - 1u) / GROUP_THREADS;
        for (int i = 0; i < n; ++i) {
            const FilterParams F{mask ? mask + (size_t)i * stride : nullptr, mask_words()};
            launch_scores(xs + (size_t)i * desc.cols, s, Q.d_gy, mask ? &F : nullptr);
            if (boost) {
                using namespace boost_kernels;
                AfterParams A{};
                A.y = Q.d_gy;
                A.total = Q.d_gwords + Grouped::W_BOOST_SINK;
                A.rows = desc.rows;
                A.first_row = desc.first_row;
                A.kmin = G.kmin;
                const BoostParams B{A, boost->weight_of(i), boost->bias_of(i), boost_wide(boost->weight_of(i), boost->bias_of(i))};
                hipLaunchKernelGGL(boost_cut_kernel, dim3(rows_grid(desc.rows, BOOST_THREADS, BOOST_LANE_ROWS)), dim3(BOOST_THREADS), 0, s, B);
            }
            (void)hipMemsetAsync(Q.d_gwords, 0, (Grouped::W_NONEMPTY + 1u) * 4, s);  // (the histogram and the non-empty-group counter)
            hipLaunchKernelGGL(group_best_kernel, dim3(best_grid), dim3(GROUP_THREADS), 0, s, G);
            hipLaunchKernelGGL(group_split_kernel, dim3(split_grid), dim3(GROUP_THREADS), 0, s, G);
            launch_radix_passes(R, Q.n_groups, s);
            S.out_idx = out_idx + (size_t)i * out_stride;
            S.out_val = out_val + (size_t)i * out_stride;
            hipLaunchKernelGGL(select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, S);
            I.idx = S.out_idx;
            I.grp = out_grp + (size_t)i * out_stride;
            I.n_out = out_n + (size_t)i * n_stride;
            hipLaunchKernelGGL(group_ids_kernel, dim3(((uint32_t)desc.k + GROUP_THREADS - 1u) / GROUP_THREADS), dim3(GROUP_THREADS), 0, s, I);
        }
    }
    // The scratch of the search-after path, allocated by its first call.
    hipError_t ensure_after() {
        After &Q = after;
        const size_t rows = std::max<size_t>(desc.rows, 1);
        if (!Q.d_ay) {
            if (const hipError_t e = alloc_ninf_scores(Q.d_ay)) return e;
        }
        if (!Q.d_acand) {
            if (const hipError_t e = alloc(Q.d_acand, rows * 8)) return e;
        }
        if (!Q.d_awords) {
            if (const hipError_t e = alloc(Q.d_awords, (size_t)SelectWords::N_WORDS * 4, Mem::Device, 0)) return e;
        }
        if (!Q.d_aout) {
            if (const hipError_t e = alloc(Q.d_aout, (size_t)After::N_OUT * 4, Mem::Device, 0)) return e;
        }
        return hipSuccess;
    }
    // A sequence of search-after queries (query i: x = xs + i * cols, cursor = cursors + i or START, mask = mask + i * stride words or
    // none; results at out_* + i * out_stride, n / total / next at their arrays' entry i where given), complete in stream
    // order when this returns: per query the SpMV-only kernel, the cut at the cursor, the radix select over the rows that remain, the
    // selection kernel and the page's bookkeeping. No exchange set, record, verdict, carried threshold or deferred selection is read
    // or written: the SpMV-only kernels touch none, and the selection kernel is given this path's own words. Only mat.launch_counter
    // moves. With a boost (tkspmv_enqueue_boosted) boost_cut_kernel takes the cut's place: the transform, the cut and the count in one
    // pass; everything behind it reads the transformed scores.
    void launch_after(const float *xs, int n, const tkspmv_cursor *cursors, const uint32_t *mask, size_t stride, uint32_t *out_idx, float *out_val,
                      size_t out_stride, uint32_t *out_n, uint32_t *out_total, tkspmv_cursor *out_next, hipStream_t s, const BoostSpec *boost = nullptr) {
        using namespace after_kernels;
        using namespace boost_kernels;
        static_assert(sizeof(AfterCursor) == sizeof(tkspmv_cursor) && sizeof(tkspmv_cursor) == 16, "the device reads tkspmv_cursor as four words");
        static_assert(BOOST_THREADS == AFTER_THREADS && BOOST_LANE_ROWS == AFTER_LANE_ROWS, "the two cut kernels share one grid");
        const After &Q = after;
        AfterParams A{};
        A.y = Q.d_ay;
        A.total = Q.d_awords + After::W_TOTAL;
        A.rows = desc.rows;
        A.first_row = desc.first_row;
        A.kmin = order_key(desc.min_score);
        const RadixParams R = radix_params(Q.d_ay, desc.rows, (uint32_t)desc.k, A.kmin, Q.d_awords, Q.d_acand, desc.rows);
        SelectParams S = array_select_params(Q.d_awords, Q.d_acand, desc.rows);  // (a candidate is a local row)
        AfterFinishParams Z{};
        Z.total = A.total;
        Z.k = (uint32_t)desc.k;
        const uint32_t cut_grid = rows_grid(desc.rows, AFTER_THREADS, AFTER_LANE_ROWS);
        for (int i = 0; i < n; ++i) {
            const FilterParams F{mask ? mask + (size_t)i * stride : nullptr, mask_words()};
            launch_scores(xs + (size_t)i * desc.cols, s, Q.d_ay, mask ? &F : nullptr);
            (void)hipMemsetAsync(Q.d_awords, 0, 4 * 256 * 4, s);  // (the histogram alone: after_finish_kernel zeroes W_TOTAL itself)
            A.cursor = cursors ? reinterpret_cast<const AfterCursor *>(cursors + i) : nullptr;
            if (boost) {
                const BoostParams B{A, boost->weight_of(i), boost->bias_of(i), boost_wide(boost->weight_of(i), boost->bias_of(i))};
                hipLaunchKernelGGL(boost_cut_kernel, dim3(cut_grid), dim3(BOOST_THREADS), 0, s, B);
            } else {
                hipLaunchKernelGGL(after_cut_kernel, dim3(cut_grid), dim3(AFTER_THREADS), 0, s, A);
            }
            launch_radix_passes(R, desc.rows, s);
            S.out_idx = out_idx + (size_t)i * out_stride;
            S.out_val = out_val + (size_t)i * out_stride;
            hipLaunchKernelGGL(select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, S);
            Z.idx = S.out_idx;
            Z.val = S.out_val;
            Z.n_out = out_n ? out_n + i : nullptr;
            Z.total_out = out_total ? out_total + i : nullptr;
            Z.next = out_next ? reinterpret_cast<AfterCursor *>(out_next + i) : nullptr;
            hipLaunchKernelGGL(after_finish_kernel, dim3(1), dim3(AFTER_FINISH_THREADS), 0, s, Z);
        }
    }
    // What the two boosted threshold forms share per query: the SpMV-only kernel into the search-after path's array, and the array
    // kernel's view of it (the query's boost and threshold).
    boost_forms::ScanParams boosted_scan(const float *xs, int i, const float *thresholds, const BoostSpec &boost, const uint32_t *mask, size_t stride,
                                         hipStream_t s) {
        const FilterParams F{mask ? mask + (size_t)i * stride : nullptr, mask_words()};
        launch_scores(xs + (size_t)i * desc.cols, s, after.d_ay, mask ? &F : nullptr);
        boost_forms::ScanParams S{};
        S.y = after.d_ay;
        S.weight = boost.weight_of(i);
        S.bias = boost.bias_of(i);
        S.threshold = thresholds + i;
        S.wide = boost_wide(S.weight, S.bias);
        S.rows = desc.rows;
        S.first_row = desc.first_row;
        return S;
    }
    // n boosted range queries (launch_range's queries and outputs, read on the boosted score of launch_after's boost), complete in stream
    // order when this returns: the counters are zeroed in front, then per query the SpMV-only kernel and boosted_hits_kernel over its
    // scores. No exchange set, record, verdict, carried threshold or deferred selection is read or written: only mat.launch_counter moves.
    void launch_boosted_range(const float *xs, int n, const float *thresholds, const BoostSpec &boost, const uint32_t *mask, size_t stride, uint32_t *idx,
                              float *val, uint32_t capacity, uint32_t *counts, hipStream_t s) {
        using namespace boost_forms;
        (void)hipMemsetAsync(counts, 0, (size_t)n * 4, s);
        const uint32_t grid_rows = rows_grid(desc.rows, BOOST_THREADS, BOOST_LANE_ROWS);
        for (int i = 0; i < n; ++i) {
            HitsParams H{};
            H.S = boosted_scan(xs, i, thresholds, boost, mask, stride, s);
            H.idx = idx ? idx + (size_t)i * capacity : nullptr;
            H.val = val ? val + (size_t)i * capacity : nullptr;
            H.capacity = capacity;
            H.count = counts + i;
            hipLaunchKernelGGL(boosted_hits_kernel, dim3(grid_rows), dim3(BOOST_THREADS), 0, s, H);
        }
    }
    // n boosted facet queries (launch_facets' queries and outputs, read on the boosted score), complete in stream order when this
    // returns: counts, best and totals are zeroed in front, then per query the SpMV-only kernel and boosted_bins_kernel, then
    // launch_facets' closing launch. The regime: calls of at most min(FACET_LDS_BINS, BINS_LDS_CAP) bins deposit in LDS -- on a grid of
    // two workgroups per CU where every workgroup sweeps more than 256 bins --, calls of more bins with global atomics.
    void launch_boosted_facets(const float *xs, int n, const float *thresholds, const BoostSpec &boost, const uint32_t *mask, size_t stride,
                               const uint32_t *labels, uint32_t n_bins, uint32_t *counts, tkspmv_facet_best *best, uint32_t *totals, hipStream_t s) {
        using namespace boost_forms;
        const size_t n_out = (size_t)n * n_bins;
        if (n_out) (void)hipMemsetAsync(counts, 0, n_out * 4, s);
        if (best && n_out) (void)hipMemsetAsync(best, 0, n_out * 8, s);
        if (totals) (void)hipMemsetAsync(totals, 0, (size_t)n * 4, s);
        const bool in_lds = n_bins <= std::min(range.facet_lds_bins, BINS_LDS_CAP);
        uint32_t grid_rows = rows_grid(desc.rows, BOOST_THREADS, BOOST_LANE_ROWS);
        if (in_lds && n_bins > 256u) grid_rows = std::min(grid_rows, std::max(1u, info.num_cus) * 2u);
        for (int i = 0; i < n; ++i) {
            BinsParams B{};
            B.S = boosted_scan(xs, i, thresholds, boost, mask, stride, s);
            B.labels = labels;
            B.wide_labels = (reinterpret_cast<uintptr_t>(labels) & 15u) == 0u ? 1u : 0u;
            B.n_bins = n_bins;
            B.in_lds = in_lds ? 1u : 0u;
            B.counts = counts + (size_t)i * n_bins;
            B.best = best ? reinterpret_cast<unsigned long long *>(best) + (size_t)i * n_bins : nullptr;
            B.total = totals ? totals + i : nullptr;
            hipLaunchKernelGGL(boosted_bins_kernel, dim3(grid_rows), dim3(BOOST_THREADS), in_lds ? (size_t)n_bins * 12u : 0u, s, B);
        }
        if (best && n_out) {
            const uint32_t cgrid = (uint32_t)std::min<size_t>((n_out + 255u) / 256u, 16384u);
            hipLaunchKernelGGL(facet_close_kernel, dim3(cgrid), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(best), (unsigned long long)n_out);
        }
    }
    // The fused launch hands its result to the host itself: the pinned block, a new epoch, the start stamp (tkspmv_run).
    void hand_to_host(SelectParams &S) {
        S.host_out = host.h_res_dev;
        S.host_epoch = ++host.host_epoch;
        S.t_start = host.d_tstart;
    }
    void launch_stream(const float *x, uint32_t *out_idx, float *out_val, hipStream_t s, bool to_host = false, const FilterParams *F = nullptr) {
        StreamParams P = stream_params(x);
        SelectParams S = select_params(out_idx, out_val);
        if (to_host) hand_to_host(S);
        ++mat.launch_counter;
        launch_stream_kernel(false, F, s, P, S);
    }
    // One query through single_kernel (local thresholds, checked): the result is exact iff the status word / host flag says the
    // check passed; otherwise the caller runs launch_stream, whose result is exact on its own.
    void launch_single(const float *x, uint32_t *out_idx, float *out_val, hipStream_t s, bool to_host) {
        StreamParams P = stream_params(x);
        SelectParams S = select_params(out_idx, out_val);
        if (to_host) hand_to_host(S);
        LocalParams G{};
        G.slots = single.d_lslots;
        G.used = single.d_lused;
        G.wg_prior = single.d_lprior;
        G.prior_block = reinterpret_cast<uint32_t *>(single.d_lprior + grid);
        G.status = single.d_lstatus;
        G.ready = single.d_lready;
        G.epoch = (uint32_t)(single.single_launches + 1u) | 0x80000000u;  // (never 0, never the previous launch's)
        G.mode = local.single_mode;
        G.beta = local.local_beta;
        G.trace = diag.trace_slot(mat.launch_counter);
        ++mat.launch_counter;
        ++single.single_launches;
        hipLaunchKernelGGL(kern.single, dim3(grid), dim3(512), 0, s, P, S, G);
    }
    void launch_query_radix(const float *x, uint32_t *out_idx, float *out_val, hipStream_t s, const FilterParams *F = nullptr) {
        launch_scores(x, s, radix.d_rscores, F);
        RadixParams R{};
        R.scores = radix.d_rscores;
        R.rows = desc.rows;
        R.k = (uint32_t)desc.k;
        R.kmin = order_key(desc.min_score);
        R.hist = radix.d_rhist;
        R.ovf_cand = ex.st[0].ovf;
        R.ovf_count = ex.st[0].ovf_count;
        R.ovf_cap = ex.ovf_cap;
        if (radix.approx_parts) {
            PartitionParams Q{};
            Q.scores = radix.d_rscores;
            Q.rows = desc.rows;
            Q.per = (desc.rows + (uint32_t)desc.partitions - 1u) / (uint32_t)desc.partitions;  // ceil(N / P): host_spmv_bscsr.cpp:136
            Q.k_part = (uint32_t)(desc.k_per_partition > 0 ? desc.k_per_partition : desc.k);
            Q.kmin = R.kmin;
            Q.ovf_cand = R.ovf_cand;
            Q.ovf_count = R.ovf_count;
            Q.ovf_cap = ex.ovf_cap;
            hipLaunchKernelGGL(partition_topk_kernel, dim3((uint32_t)desc.partitions), dim3(RADIX_THREADS), 0, s, Q);
        } else {
            (void)hipMemsetAsync(radix.d_rhist, 0, 4 * 256 * 4, s);
            launch_radix_passes(R, desc.rows, s);
        }
        SelectParams S = select_params(out_idx, out_val, 0);
        S.use_gmax = 0u;  // no threshold word in this path
        S.out_scale = 1.0f;  // the scores kernel already wrote final scores
        hipLaunchKernelGGL(select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, S);
    }
    void launch_scores(const float *x, hipStream_t s, float *dst = nullptr, const FilterParams *F = nullptr) {
        StreamParams P = stream_params(x);
        if (dst) P.scores = dst;
        SelectParams S = select_params(host.d_out_idx, host.d_out_val);
        ++mat.launch_counter;  // the stream copies rotate per query here too (cache-defeat mode)
        launch_stream_kernel(true, F, s, P, S);
    }
    void launch_select(uint32_t *out_idx, float *out_val, hipStream_t s, int set = 0) const {
        SelectParams S = select_params(out_idx, out_val, set);
        S.unit_inv_in = ex.st[set].unit_inv;  // written by the (unfused) stream kernel of that query
        hipLaunchKernelGGL(select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, S);
    }
    // Does the host-visible result block add up to the checksum its writer left behind the flag (result_checksum_term)? The block
    // is written with relaxed system-scope stores; the flag alone proves nothing by the memory model.
    bool result_block_complete(uint32_t epoch) const {
        const size_t k = (size_t)desc.k;
        const volatile uint32_t *r = host.h_res;
        // (word 2k + 5: the status of single_kernel's check. A FAILED check writes no payload -- the block still holds the previous
        //  query's list -- and its checksum covers the epoch and the status alone: summing the stale payload here would never match,
        //  and every failed check would cost tkspmv_run its 2 s flag timeout before the repair)
        if (r[2 * k + 5] != 0u) return r[2 * k + 4] == epoch * 0x9E3779B1u + 0xBADC0DE5u;
        uint32_t sum = epoch * 0x9E3779B1u;
        for (size_t i = 0; i < k; ++i) sum += result_checksum_term(r[i], r[k + i], (uint32_t)i);
        return r[2 * k + 4] == sum;
    }
    // tkspmv_set_query enqueues the upload of x on the engine's stream and does not wait for it. A launch that reads d_x from
    // ANOTHER stream (tkspmv_enqueue with a caller's stream and dev_x = NULL) has no ordering against that copy -- the
    // engine's stream is non-blocking -- so it waits for the event recorded behind the copy.
    hipError_t order_x(const float *x, hipStream_t s) const {
        if (x != host.d_x || !host.x_pending || s == stream || host.bar_x) return hipSuccess;  // (bar_x: the host wrote x itself, nothing is enqueued)
        return hipStreamWaitEvent(s, ev2, 0);
    }
    // dev_xs = NULL names the vector tkspmv_set_query / set_query_device installed: the call is then for that one query.
    int resolve_query(const float *&dev_xs, int32_t count, std::string &err) const {
        if (dev_xs) return TKSPMV_OK;
        if (count != 1) return fail(err, TKSPMV_ERR_INVALID, "dev_xs = NULL takes the installed query vector: count must be 1");
        if (!host.d_x_cur) return fail(err, TKSPMV_ERR_STATE, "no query vector installed (call tkspmv_set_query first)");
        dev_xs = host.d_x_cur;
        return TKSPMV_OK;
    }
    // use_filter of the host forms names the mask tkspmv_set_filter installed: that mask, or NULL without use_filter. A missing mask
    // is answered with `status`: INVALID by the tkspmv_run_* forms, STATE by tkspmv_nearest and tkspmv_col_stats.
    int installed_mask(int32_t use_filter, const uint32_t *&mask_out, std::string &err, int status = TKSPMV_ERR_INVALID) const {
        if (use_filter && !filter.have_filter) return fail(err, status, "use_filter without an installed allow-mask (tkspmv_set_filter)");
        mask_out = use_filter ? filter.d_filter : nullptr;
        return TKSPMV_OK;
    }
    // The scope test of the whole-matrix calls, which all share the row vectors' scope: UNSUPPORTED, the call's prefix in front of the reason.
    static constexpr const char *STATS_SCOPE = "row statistics share the row vectors' scope: ", *ASSIGN_SCOPE = "assignment shares the row vectors' scope: ",
                                *SUMS_SCOPE = "label sums share the row vectors' scope: ";
    int row_scope(std::string &err, const char *prefix = "") const {
        const char *why = row_vectors_unsupported();
        return why ? fail(err, TKSPMV_ERR_UNSUPPORTED, std::string(prefix) + why) : TKSPMV_OK;
    }
    // A host form's own launches on the engine's stream, and the wait for them. No result is read and no result buffer written, so the
    // engine need not be settled (wait_idle, which tkspmv_row_vectors and tkspmv_run_similar call, settles it).
    template <class Launch>
    hipError_t launch_and_wait(Launch launch) const {
        launch();
        const hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    }
    // tkspmv_assign (n = 1) and tkspmv_nearest: n labels and scores per row for `count` host vectors. Chunks of vectors: up, the chunk's
    // launches -- launch(xs, qc, q0, labels, scores): the chunk's qc vectors are the call's vectors q0 .. --, wait (the next chunk
    // overwrites the vectors); then the results down. The scratch grows behind a wait for the stream (an earlier call's chunks are long
    // complete: the host forms wait themselves).
    template <class Launch>
    int assign_host(const float *host_xs, int32_t count, uint32_t n, uint32_t *host_labels, float *host_scores, std::string &err, Launch launch) {
        if (desc.rows == 0u) return TKSPMV_OK;
        HIP_TRY(hipSetDevice(device));
        Assign &A = assign;
        const size_t cols = desc.cols, rows = desc.rows, x_bytes = std::max<size_t>(cols, 1) * 4;
        const uint32_t want = (uint32_t)std::min<size_t>((size_t)count, std::max<size_t>(1, Assign::ASSIGN_MAX_BYTES / x_bytes));
        if (n > A.as_n || want > A.as_cap) HIP_TRY(hipStreamSynchronize(stream));
        if (n > A.as_n) HIP_TRY(grow_scratch(A.as_n, n, {{(void **)&A.d_as_labels, rows * n * 4}, {(void **)&A.d_as_scores, rows * n * 4}}));
        if (want > A.as_cap) HIP_TRY(grow_scratch(A.as_cap, want, {{(void **)&A.d_as_xs, (size_t)want * x_bytes}}));
        for (int32_t q0 = 0; q0 < count; q0 += (int32_t)A.as_cap) {
            const int32_t qc = std::min<int32_t>((int32_t)A.as_cap, count - q0);
            HIP_TRY(hipMemcpy(A.d_as_xs, host_xs + (size_t)q0 * cols, (size_t)qc * cols * 4, hipMemcpyHostToDevice));
            HIP_TRY(launch_and_wait([&] { launch(A.d_as_xs, qc, (uint32_t)q0, A.d_as_labels, A.d_as_scores); }));
        }
        HIP_TRY(hipMemcpy(host_labels, A.d_as_labels, rows * n * 4, hipMemcpyDeviceToHost));
        if (host_scores) HIP_TRY(hipMemcpy(host_scores, A.d_as_scores, rows * n * 4, hipMemcpyDeviceToHost));
        return TKSPMV_OK;
    }
    // A call's own masks are mask_stride_words apart; the installed mask, or none, serves every query of the call.
    static size_t stride_of(const uint32_t *dev_mask, int64_t mask_stride_words) { return dev_mask ? (size_t)mask_stride_words : 0u; }
    // Checks of trusted batch launches still pending under REPAIR=host: a late repair would write the engine-owned result pair
    // after the queries about to be enqueued did (own: they write it). Settle them now (the host waits for the engine's stream once).
    int settle_before_owned_result(bool own, std::string &err) { return own && !trust.pending_checks.empty() ? wait_idle(err) : TKSPMV_OK; }
    // The tail of a host form that ran the installed query vector: the host waits and looks at the verdicts, and nothing reads the
    // staging copy of x any more. (tkspmv_run_match reads no query vector and leaves x_pending alone: it calls wait_idle itself.)
    int finish_host_form(std::string &err) {
        if (const int st = wait_idle(err)) return st;
        host.x_pending = false;
        return TKSPMV_OK;
    }
    // Replaces the buffers of a scratch set that grows on demand (run_range, run_similar) by larger ones: all released, then all
    // allocated; `cap` is 0 while the set is incomplete. The caller has waited for whatever used the old ones.
    struct ScratchSlot { void **p; size_t bytes; };
    hipError_t grow_scratch(uint32_t &cap, uint32_t want, std::initializer_list<ScratchSlot> slots) {
        for (const ScratchSlot &b : slots) {
            release(*b.p);
            *b.p = nullptr;
        }
        cap = 0u;
        for (const ScratchSlot &b : slots) {
            uint8_t *q = nullptr;
            if (const hipError_t e = alloc(q, b.bytes)) return e;
            *b.p = q;
        }
        cap = want;
        return hipSuccess;
    }
};

uint64_t algorithmic_bytes(uint64_t nnz, uint32_t rows, uint32_t cols, uint32_t vbytes, int k) {
    // value + 16-bit column per nnz; 4 B of row-delimiting metadata per row; x once; k pairs out.
    return nnz * (uint64_t)(vbytes + 2) + (uint64_t)rows * 4 + (uint64_t)cols * vbytes + (uint64_t)k * 8;
}

void fill_info(const PackedMatrix &pm, int k, tkspmv_info *out) {
    std::memset(out, 0, sizeof(*out));
    out->rows = pm.rows;
    out->cols = pm.cols;
    out->nnz = pm.nnz;
    out->packed_entries = pm.packed_entries;
    out->packed_bytes = pm.stream_bytes() + pm.side_bytes();
    out->algorithmic_bytes = algorithmic_bytes(pm.nnz, pm.rows, pm.cols, value_bytes(pm.precision), k);
    out->n_packets = pm.n_packets;
    out->packet_entries = pm.packet_entries;
    out->n_wave_partitions = (uint32_t)pm.part_first.size();
    out->packets_per_partition = pm.packets_per_partition;
    out->k = k;
    // (the bit-packed narrow fixed-point stream is a layout of TKSPMV_FIXED, not a precision of the API)
    out->precision = (pm.precision == Precision::FIXED20 || pm.precision == Precision::FIXED26) ? (int32_t)Precision::FIXED
                                                       : (pm.precision == Precision::F32C12 ? (int32_t)Precision::F32 : (int32_t)pm.precision);
    out->fixed_width = pm.fixed_width;
    out->batch_stream_bytes = pm.stream_bytes();  // (an engine that keeps compact copies says so in fill_engine_info)
    out->batch_packet_bytes = pm.packet_bytes;
}

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int use_device(int device, std::string &err) {
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    return TKSPMV_OK;
}

Engine::~Engine() {
    if (!impl_) return;
    EngineImpl &m = *impl_;
    (void)hipSetDevice(m.device);
    for (hipStream_t s : {m.stream, m.multi.side}) if (s) (void)hipStreamSynchronize(s);
    for (const EngineImpl::Owned &b : m.owned) (void)(b.pinned ? hipHostFree(b.p) : hipFree(b.p));
    for (hipEvent_t e : {m.ev0, m.ev1, m.ev2, m.multi.ev_fork, m.multi.ev_join}) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {m.multi.side, m.stream}) if (s) (void)hipStreamDestroy(s);
    delete impl_;
}

// Small matrices (the shards of a strong-scaled run): a query streams in less time than one selection takes and than a
// device-wide threshold needs to form. They get 4 selector workgroups, partitions from 1-2 packets up (every wave streams:
// twice the loads in flight; wbscsr.hpp: min_packets_per_partition_for) and workgroup-local thresholds. With pacing by rank
// (setup_verdicts) the same settings win up to LOCAL_MATRIX_PACKETS -- the headline's 1M rows included; beyond, the device-wide
// exchange is as fast and checks nothing. Returns the selector workgroups of a batch launch for this matrix and geometry
// (TKSPMV_SELECTORS overrides; the matrix unknown -- nnz = 0 --: 1). TKSPMV_SMALL_PACKETS: both limits (0: round 2's behaviour).
// (fp32 and fp16 values: every size, wbscsr.hpp; byte and fixed-point values keep round 4's limit -- their kernels are bound by
//  arithmetic, and there the local thresholds lose beyond it: Q1.7 bytes at 1M x 512 x 40, 154k packets: 33.0 against 24.7 us)
static uint64_t local_matrix_packets(int32_t precision) {
    return small_packets_limit((precision == TKSPMV_F32 || precision == TKSPMV_F16) ? LOCAL_MATRIX_PACKETS : 100000ull);
}
static uint32_t small_matrix_settings(const tkspmv_desc &d, uint32_t grid, bool defer_capable, uint32_t C, bool *small_out) {
    const uint64_t packets_lb = d.nnz / (64u * (uint64_t)std::max(C, 1u));
    // (partitions with k <= k_per_partition: the union of the per-partition lists holds the global top-k -- the ordinary kernels'
    //  result IS the partitioned one, check_desc --, so such engines take the settings of an unpartitioned one: BASELINE configs[2])
    const bool plain_topk = d.partitions <= 1 || d.k <= (d.k_per_partition > 0 ? d.k_per_partition : d.k);
    const bool small = defer_capable && grid >= 64u && d.nnz != 0 && d.cols <= 1024u && d.impl == TKSPMV_IMPL_STREAM && d.multi_q == 0 &&
                       plain_topk && packets_lb <= local_matrix_packets(d.precision) && !opt("MULTI_Q");
    if (small_out) *small_out = small;
    uint32_t n = (uint32_t)opt_int("SELECTORS", small ? 4 : 1, 1, 8);
    if (!defer_capable || grid < 2u * n) n = 1u;
    return n;
}

// A device buffer of one host function (a measurement's inputs, a check's read-back): freed on every return path.
template <class T> struct ScratchBuffer {
    T *p = nullptr;
    ~ScratchBuffer() { if (p) (void)hipFree(p); }
};
// The events of one host function (a measurement's brackets), likewise.
struct ScratchEvents {
    std::vector<hipEvent_t> e;
    explicit ScratchEvents(size_t n) : e(n, nullptr) {}
    ~ScratchEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// tkspmv_create: create_impl runs the stages below in order. Each returns a TKSPMV_* status; what the engine keeps goes into
// EngineImpl, what only a later stage needs into Setup. Buffers go through EngineImpl::alloc: ~Engine frees them on every path.
struct Setup {
    const PackedMatrix *prepacked;  // tkspmv_pack / a .tkspmv file; NULL: pack d's COO
    uint32_t num_cus = 0;
    size_t lds_per_cu = 0;
    uint32_t waves_per_wg = 0;      // streaming waves; one more wave per workgroup serves the exchange
    uint32_t C = 0;                 // entries per lane
    bool defer_capable = false;     // workgroup 0 of a back-to-back launch can select the previous query
    bool small_matrix = false;      // small_matrix_settings()
    uint32_t n_stream_waves = 0;    // streaming waves of a sequence launch
    uint32_t n_parts_hint = 0;      // wave partitions the packer cuts
    bool packed_on_device = false;  // the stream was built by device_pack.hip
    uint32_t *d_coo_col = nullptr;  // the COO's columns and values, kept in HBM between the two device packers
    float *d_coo_val = nullptr;
    uint32_t pack_us = 0;           // time of the packing step (upload of the COO included when on the device)
    uint32_t sell_pack_us = 0;      // packing of the wave-sliced ELL copy (multi-query engines)
    uint64_t sell_bytes = 0;
    int sell_values = 0;            // values of that copy: 0 fp32; 1 Q1.7 bytes (TKSPMV_Q1_7_F32: 768-byte chunks); 2 ... with 12-bit column words (640-byte chunks, at most 1022 columns)
};

// The descriptor alone: no device call before these checks (tests/test_capi.py::test_argument_validation_before_device).
static int check_desc(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    if (d.k < 1 || d.k > TKSPMV_MAX_K) return fail(err, TKSPMV_ERR_INVALID, "k must be in [1, 1024]");
    if (d.cols == 0 || d.cols > TKSPMV_MAX_COLS) return fail(err, TKSPMV_ERR_INVALID, "cols must be in [1, 16384]");
    if (d.precision != TKSPMV_F32 && d.precision != TKSPMV_Q1_7 && d.precision != TKSPMV_Q1_7_WIDE &&
        d.precision != TKSPMV_F16 && d.precision != TKSPMV_FIXED && d.precision != TKSPMV_Q1_7_F32)
        return fail(err, TKSPMV_ERR_INVALID, "unknown precision");
    if (d.impl == 3)  // (rounds 2-4: a resident kernel serving tkspmv_run; slower than a launch per query since round 4, removed in round 5)
        return fail(err, TKSPMV_ERR_UNSUPPORTED, "impl 3 (the resident kernel) was removed: tkspmv_run through impl 0 (single_kernel) is faster");
    if (d.impl != TKSPMV_IMPL_STREAM && d.impl != TKSPMV_IMPL_ROW_PER_LANE && d.impl != TKSPMV_IMPL_SCORES_SELECT)
        return fail(err, TKSPMV_ERR_INVALID, "unknown impl (0 = stream, 1 = row per lane, 2 = scores + select)");
    if (d.precision == TKSPMV_FIXED ? (d.fixed_width != 0 && (d.fixed_width < 8 || d.fixed_width > 32)) : d.fixed_width != 0)
        return fail(err, TKSPMV_ERR_INVALID, "fixed_width must be 0 (= 32) or in [8, 32] for TKSPMV_FIXED, and 0 for every other precision");
    if (d.precision != TKSPMV_F32 && d.nnz_per_lane == 8)
        return fail(err, TKSPMV_ERR_UNSUPPORTED, "the reduced precisions are built for nnz_per_lane = 4 only");
    if (d.partitions > 1) {
        // The reference keeps k_per_partition (its compile-time K) candidates per row partition and merges them on
        // the host (host_spmv_bscsr.cpp:399-448). For k <= k_per_partition the union of the per-partition lists
        // contains the global top-k, so the partitioned result IS the exact one computed by the ordinary kernels. With
        // k > k_per_partition (the FPGA design's lossy regime: 32 partitions x K = 8 lists answering k = 100) the engine
        // reproduces the reference's approximate union: partition_topk_kernel.
        const int kpp = d.k_per_partition > 0 ? d.k_per_partition : d.k;
        if (kpp > TKSPMV_MAX_K || d.partitions > 65535) return fail(err, TKSPMV_ERR_INVALID, "partitions must be <= 65535 and k_per_partition <= 1024");
        m.radix.approx_parts = d.k > kpp;
    }
    return TKSPMV_OK;
}

// The device, the launch geometry (grid, block), the selector workgroups and the partitions the packer aims at.
static int setup_geometry(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(err, TKSPMV_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    int dev = d.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= ndev) return fail(err, TKSPMV_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(dev));
    m.device = dev;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    S.num_cus = (uint32_t)prop.multiProcessorCount;
    S.lds_per_cu = (size_t)prop.maxSharedMemoryPerMultiProcessor;
    m.desc = d;
    m.desc.row = m.desc.col = nullptr;
    m.desc.val = nullptr;
    m.block = d.threads_per_wg > 0 ? (uint32_t)d.threads_per_wg : 512u;
    if (m.block % 64 || m.block > 512 || m.block < 64)
        return fail(err, TKSPMV_ERR_INVALID, "threads_per_wg must be a multiple of 64, at most 512");
    const uint32_t waves_per_cu = d.waves_per_cu > 0 ? (uint32_t)d.waves_per_cu : 16u;
    S.waves_per_wg = m.block / 64;
    m.grid = std::max(1u, S.num_cus * waves_per_cu / S.waves_per_wg);
    if ((uint64_t)m.grid * WG_SLOTS > (uint64_t)SEL_PER_THREAD * SEL_THREADS)
        return fail(err, TKSPMV_ERR_INVALID, "launch geometry too large: waves_per_cu * num_cus / waves_per_wg must be <= 1024 workgroups");
    S.C = entries_per_lane_of(d);
    // Deferred selection gives workgroup 0 of a back-to-back launch to the previous query's selection: one
    // partition per streaming wave of the remaining grid - 1 workgroups.
    S.defer_capable = m.grid >= 2 && (uint64_t)m.grid * WG_SLOTS <= (uint64_t)SEL_PER_THREAD * (m.block + 64);
    // Small matrices (the shards of a strong-scaled run) get 4 selector workgroups, shorter partitions and -- decided in
    // setup_verdicts, once the partitions are known -- workgroup-local thresholds: small_matrix_settings().
    m.batch.n_sel_wg = small_matrix_settings(d, m.grid, S.defer_capable, S.C, &S.small_matrix);
    if (S.prepacked && S.prepacked->part_first.size() > (size_t)(m.grid - m.batch.n_sel_wg) * S.waves_per_wg) m.batch.n_sel_wg = 1u;
    S.n_stream_waves = (m.grid - (S.defer_capable ? m.batch.n_sel_wg : 0u)) * S.waves_per_wg;
    // (TKSPMV_PARTITIONS_HINT: measurement aid of the load-only probe -- more partitions than waves; such an engine runs no queries)
    S.n_parts_hint = (uint32_t)opt_int("PARTITIONS_HINT", S.n_stream_waves);
    return TKSPMV_OK;
}

// The packed matrix: a prepacked one checked against the descriptor, or d's COO packed on the device or the host; its info and
// whether its partition table is uniform.
static int pack_matrix(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    if (S.prepacked) {
        // A matrix packed earlier (tkspmv_pack / a .tkspmv file): it must describe the same problem and must not have
        // more partitions than this launch geometry has streaming waves (the batch kernel gives every wave one).
        const PackedMatrix &q = *S.prepacked;
        const bool fixed_either = d.precision == TKSPMV_FIXED && (q.precision == Precision::FIXED || q.precision == Precision::FIXED20 || q.precision == Precision::FIXED26);
        const bool f32_either = d.precision == TKSPMV_F32 && (q.precision == Precision::F32 || q.precision == Precision::F32C12);
        if (q.rows != d.rows || q.cols != d.cols || (!fixed_either && !f32_either && q.precision != stream_precision(d.precision)) ||
            q.C != S.C || q.fixed_width != fixed_width_of(d))
            return fail(err, TKSPMV_ERR_INVALID, "the packed matrix does not match the descriptor (rows, cols, precision or entries per lane)");
        if (q.part_first.size() > S.n_stream_waves)
            return fail(err, TKSPMV_ERR_UNSUPPORTED, "the packed matrix has more wave partitions than this GPU's launch geometry has streaming waves: pack it "
                                                     "again with tkspmv_pack(desc, " + std::to_string(S.n_stream_waves) + ", ...)");
        if (q.packets.size() != q.stream_bytes() || q.pkt_row.size() != q.n_packets) return fail(err, TKSPMV_ERR_INVALID, "the packed matrix is incomplete");
        m.pm = q;  // copy: the engine drops its host copy of the stream after the upload
        m.desc.nnz = q.nnz;
    } else {
        // The packer runs on the device by default (device_pack.hip: same bytes as the host packer, which stays available
        // with TKSPMV_DEVICE_PACK=0 and serves tkspmv_pack / the .tkspmv files).
        const bool on_device = d.nnz > 0 && opt_int("DEVICE_PACK", 1) != 0;
        const uint32_t min_packets = min_packets_per_partition_for(d.nnz, S.C, d.cols);
        const auto t_pack = std::chrono::steady_clock::now();
        std::string perr;
        int kind = 0;
        if (on_device) {
            DevicePacked dp;
            // (a multi-query engine packs the same COO a second time in setup_multi: leave its columns and values in HBM until then)
            dp.keep_coo = d.cols <= SELL_XCOLS && (d.multi_q != 0 || d.impl == TKSPMV_IMPL_ROW_PER_LANE || opt("MULTI_Q"));
            perr = pack_wbscsr_device(d.rows, d.cols, d.nnz, d.row, d.col, d.val, stream_precision_of(d), S.C,
                                      S.n_parts_hint, min_packets, fixed_width_of(d), dp, kind);
            if (perr.empty()) {
                m.pm = std::move(dp.meta);
                m.mat.d_packets = m.adopt(dp.d_packets);
                m.mat.d_pkt_row = m.adopt(dp.d_pkt_row);
                S.d_coo_col = m.adopt(dp.d_col);
                S.d_coo_val = m.adopt(dp.d_val);
                S.packed_on_device = true;
            }
        } else {
            perr = pack_wbscsr(d.rows, d.cols, d.nnz, d.row, d.col, d.val, stream_precision_of(d), S.C, S.n_parts_hint, min_packets,
                               m.pm, kind, fixed_width_of(d));
        }
        if (!perr.empty())
            return fail(err, kind == 2 ? TKSPMV_ERR_NOT_SORTED : (perr.find("failed:") != std::string::npos ? TKSPMV_ERR_DEVICE : TKSPMV_ERR_INVALID), perr);
        S.pack_us = (uint32_t)std::min<long long>(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_pack).count(), 0xFFFFFFFFll);
    }
    // A matrix without entries packs to no packets and no partitions. The launch paths divide the stream among their waves by
    // the partition table and were written for at least one partition; none of them is specified over an empty table, so such
    // an engine is refused here (a rank whose shard came out empty answers with k fillers (0, 0.0f) without an engine).
    if (m.pm.n_packets == 0)
        return fail(err, TKSPMV_ERR_INVALID, "the matrix has no entries (nnz = 0): an engine needs at least one; a row shard without entries "
                                             "contributes k fillers (0, 0.0f) to the merge and needs no engine");
    fill_info(m.pm, d.k, &m.info);
    // The packer's usual outcome is a uniform table -- every partition but the last holds packets_per_partition packets, back
    // to back --: the kernels then derive a wave's range from its partition number (no table loads at the head of a launch).
    const size_t np = m.pm.part_first.size();
    const uint32_t ppp = m.pm.packets_per_partition;
    bool uniform = np > 0 && ppp > 0 && (uint64_t)np * ppp <= 0xFFFFFFFFull && m.pm.part_count[np - 1] >= 1u && m.pm.part_count[np - 1] <= ppp;
    for (size_t p = 0; uniform && p < np; ++p)
        uniform = m.pm.part_first[p] == (uint32_t)(p * ppp) && (p + 1 == np || m.pm.part_count[p] == ppp);
    m.mat.uni_ppp = uniform ? ppp : 0u;
    m.mat.uni_last = uniform ? m.pm.part_count[np - 1] : 0u;
    return TKSPMV_OK;
}

// Threshold-exchange geometry: at least k publishing groups are needed (tau = k-th largest published maximum);
// if one group per workgroup is not enough, the waves of a workgroup are split into up to 8 groups.
// Counted on the workgroups that stream in a sequence launch (grid - 1: workgroup 0 selects). Aim for 4k groups
// where the 1024-word limit of the exchange allows: with k close to the number of groups the k-th largest maximum
// is a weak bound (k = 256 on 511 groups ran 2x slower than k = 100).
static int exchange_geometry(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    const uint32_t waves_per_wg = S.waves_per_wg, n_pub_wg = m.grid - (S.defer_capable ? m.batch.n_sel_wg : 0u);
    m.ex.gpw = 1;
    while (n_pub_wg * m.ex.gpw < 4u * (uint32_t)d.k && m.ex.gpw < 8 && m.ex.gpw < waves_per_wg && (waves_per_wg % (m.ex.gpw * 2) == 0) &&
           m.grid * m.ex.gpw * 2 <= (uint32_t)MAX_GM * 64)
        m.ex.gpw *= 2;
    m.ex.n_groups_pub = std::min<uint32_t>(m.grid * m.ex.gpw, MAX_GM * 64);
    m.ex.n_sets = (std::min<uint32_t>(n_pub_wg * m.ex.gpw, MAX_GM * 64) >= (uint32_t)d.k) ? 1u : 0u;  // 0: exchange disabled, every row >= min_score is a candidate
    if (!m.ex.n_sets) m.ex.n_groups_pub = 1;
    m.ex.ovf_cap = std::max<uint32_t>(d.rows, 1u);
    m.fmt = stream_format_of(d.precision, m.pm.precision, m.info.packet_entries, d.cols);
    if (m.fmt.c == 0) return fail(err, TKSPMV_ERR_UNSUPPORTED, "no kernel is built for this descriptor's packet stream");  // (the packers accept none)
    m.ex.cand_cap = m.fmt.xcols <= 1024 ? 2048u : 1024u;  // ListGeom<XCOLS>::CAND_CAP
    // groups (workgroup, local group) whose first wave owns a partition: wave w of streaming workgroup b streams
    // partition w * n_pub_wg + b (n_pub_wg: the streaming workgroups of a sequence launch)
    const uint32_t n_parts = (uint32_t)m.pm.part_first.size();
    m.ex.groups_with_rows = 0;
    for (uint32_t b = 0; b < n_pub_wg; ++b)
        for (uint32_t g = 0; g < m.ex.gpw; ++g) {
            const uint32_t w0 = g * waves_per_wg / m.ex.gpw;
            if ((uint64_t)w0 * n_pub_wg + b < n_parts && (uint64_t)b * m.ex.gpw + g < m.ex.n_groups_pub) ++m.ex.groups_with_rows;
        }
    if (S.C == 8 && d.cols > 1024) return fail(err, TKSPMV_ERR_UNSUPPORTED, "nnz_per_lane = 8 is only built for cols <= 1024");
    m.ex.lds_bytes = (uint32_t)std::max<size_t>(sizeof(SelectShared), (size_t)m.fmt.xcols * 4 + (size_t)m.ex.cand_cap * 8) +
                  MISC_WORDS * 4;  // all static
    return TKSPMV_OK;
}

// The engine's stream and events; the packed stream, its row and partition tables and the stream's replicas in HBM.
static int upload_matrix(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    HIP_TRY(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&m.ev0));
    HIP_TRY(hipEventCreate(&m.ev1));
    HIP_TRY(hipEventCreate(&m.ev2));
    const size_t stream_bytes = std::max<size_t>(m.pm.stream_bytes(), 256);
    if (!S.packed_on_device) {  // (the device packer has left the stream and its row table in HBM already)
        HIP_TRY(m.alloc(m.mat.d_packets, stream_bytes));
        HIP_TRY(m.alloc(m.mat.d_pkt_row, std::max<size_t>(m.pm.pkt_row.size(), 1) * 4));
        if (m.pm.stream_bytes())
            HIP_TRY(hipMemcpy(m.mat.d_packets, m.pm.packets.data(), m.pm.stream_bytes(), hipMemcpyHostToDevice));
        if (!m.pm.pkt_row.empty())
            HIP_TRY(hipMemcpy(m.mat.d_pkt_row, m.pm.pkt_row.data(), m.pm.pkt_row.size() * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(m.alloc(m.mat.d_part_first, std::max<size_t>(m.pm.part_first.size(), 1) * 4));
    HIP_TRY(m.alloc(m.mat.d_part_count, std::max<size_t>(m.pm.part_count.size(), 1) * 4));
    if (!m.pm.part_first.empty()) {
        HIP_TRY(hipMemcpy(m.mat.d_part_first, m.pm.part_first.data(), m.pm.part_first.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m.mat.d_part_count, m.pm.part_count.data(), m.pm.part_count.size() * 4, hipMemcpyHostToDevice));
    }
    if (d.stream_replicas > 1 && m.pm.stream_bytes()) {
        m.mat.d_replicas.push_back(m.mat.d_packets);
        for (int r = 1; r < d.stream_replicas; ++r) {
            uint8_t *p = nullptr;
            HIP_TRY(m.alloc(p, stream_bytes));
            HIP_TRY(hipMemcpy(p, m.mat.d_packets, m.pm.stream_bytes(), hipMemcpyDeviceToDevice));
            m.mat.d_replicas.push_back(p);
        }
    }
    // The packed stream now lives in HBM; drop the host copy.
    std::vector<uint8_t>().swap(m.pm.packets);
    std::vector<uint32_t>().swap(m.pm.pkt_row);
    return TKSPMV_OK;
}

// The host boundary -- x on the device, the BAR path, the pinned staging copy of x and result block -- and the result buffers.
static int setup_host_boundary(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    HIP_TRY(m.alloc(m.host.d_x, (size_t)d.cols * 4));
    m.host.host_path = (int)opt_int("HOST_PATH", 1);
    // Host stores into device memory (host.bar_x): only where the runtime reports a large BAR, and only after a round trip
    // has shown that a value stored by the CPU is the value a kernel reads back.
    int large_bar = 0;
    if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, m.device) != hipSuccess) large_bar = 0;
    (void)hipGetLastError();
    bool want = large_bar != 0 && m.host.host_path != 0 && opt_int("BAR_X", 1) != 0;
    if (want) {
        uint32_t *reg = nullptr;  // (the attribute is returned through the int pointer as an address)
        if (hipDeviceGetAttribute(reinterpret_cast<int *>(&reg), hipDeviceAttributeHdpMemFlushCntl, m.device) != hipSuccess) reg = nullptr;
        (void)hipGetLastError();
        m.host.hdp_flush = reg;
        want = reg != nullptr;
    }
    if (want) {
        // Four rounds with changing values: the CPU stores two words and flushes the HDP, a KERNEL loads them (a copy engine
        // reading them back proves nothing about what a kernel's loads see behind its caches) -- after a kernel of an
        // earlier round has had the old values in its caches.
        ScratchBuffer<uint32_t> back_dev;
        HIP_TRY(hipMalloc((void **)&back_dev.p, 8));
        HIP_TRY(hipMemset(m.host.d_x, 0, (size_t)d.cols * 4));
        HIP_TRY(hipDeviceSynchronize());
        volatile uint32_t *px = reinterpret_cast<volatile uint32_t *>(m.host.d_x);
        bool ok = true;
        for (uint32_t round = 0; round < 4u && ok; ++round) {
            const uint32_t a = 0x5A17C0DEu + 0x01010101u * round, b = (0xC0DE5A17u ^ d.cols) + 0x00010001u * round;
            px[0] = a;
            px[d.cols - 1] = b;
            m.host.flush_hdp();
            hipLaunchKernelGGL(bar_check_kernel, dim3(1), dim3(64), 0, nullptr, reinterpret_cast<const uint32_t *>(m.host.d_x), d.cols - 1u, back_dev.p);
            uint32_t back[2] = {0, 0};
            HIP_TRY(hipMemcpy(back, back_dev.p, 8, hipMemcpyDeviceToHost));
            ok = back[0] == (d.cols == 1 ? b : a) && back[1] == b;
        }
        m.host.bar_x = ok;
        HIP_TRY(hipMemset(m.host.d_x, 0, (size_t)d.cols * 4));
        HIP_TRY(hipDeviceSynchronize());
    }
    if (m.host.host_path) {  // pinned staging copy of x and the host-visible result block (optional: the plain path needs neither)
        const char *hx = opt("HOST_X");
        if (hx) m.host.host_x_direct = std::string(hx) == "direct" || std::string(hx) == "direct_nc";
        m.host.run_events = opt_int("RUN_EVENTS", 0) != 0;
        const unsigned flags = (hx && std::string(hx) == "direct_nc") ? (hipHostMallocMapped | hipHostMallocNonCoherent) : hipHostMallocMapped;
        (void)m.alloc(m.host.h_x, (size_t)d.cols * 4, Mem::Pinned, -1, flags);  // (none: tkspmv_set_query takes the plain path)
        if (m.host.h_x && hipHostGetDevicePointer((void **)&m.host.h_x_dev, m.host.h_x, 0) != hipSuccess) m.host.host_x_direct = false;
        if (m.alloc(m.host.h_res, ((size_t)2 * d.k + 16) * 4, Mem::Pinned, 0) != hipSuccess ||
            hipHostGetDevicePointer((void **)&m.host.h_res_dev, m.host.h_res, 0) != hipSuccess) {
            m.release(m.host.h_res);
            m.host.h_res = m.host.h_res_dev = nullptr;
        }
        (void)hipGetLastError();
    }
    HIP_TRY(m.alloc(m.host.d_out_idx, (size_t)d.k * 4, Mem::Device, 0));
    HIP_TRY(m.alloc(m.host.d_out_val, (size_t)d.k * 4, Mem::Device, 0));
    HIP_TRY(m.alloc(m.diag.d_stats, 32 * 8, Mem::Device, 0));
    m.diag.collect_stats = opt("STATS") != nullptr;
    HIP_TRY(m.alloc(m.host.d_tstart, 128, Mem::Exchange, 0));
    HIP_TRY(m.alloc(m.ex.d_done, 9 * 128, Mem::Exchange, 0));
    return TKSPMV_OK;
}

// The path: fused tail, deferred selection, the batch kernel, the scores + radix-select path.
static int choose_path(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    // Fused tail / deferred selection: one workgroup (block + 64 threads) must hold every slot in SEL_PER_THREAD
    // registers per thread.
    m.defer.fused = (uint64_t)m.grid * WG_SLOTS <= (uint64_t)SEL_PER_THREAD * (m.block + 64);
    m.defer.can_defer = S.defer_capable;
    m.defer.fused = m.defer.fused && opt_int("FUSED", 1) != 0;
    m.batch.can_batch = m.defer.can_defer && m.ex.n_sets != 0u && is_batchable(m.fmt);
    m.batch.can_batch = m.batch.can_batch && opt_int("BATCH", 1) != 0;
    // Large k: the scores + radix-select path wherever the threshold exchange is off or next to useless (k above
    // 3/8 of the publishing groups: measured cross-over on the BASELINE matrix, tools/k_probe.py). TKSPMV_RADIX=0/1 forces.
    m.radix.use_radix = m.ex.n_sets == 0u || (uint64_t)d.k * 8u > (uint64_t)m.ex.n_groups_pub * 3u || d.impl == TKSPMV_IMPL_SCORES_SELECT;
    m.radix.use_radix = opt_int("RADIX", m.radix.use_radix) != 0;
    if (m.radix.approx_parts) m.radix.use_radix = true;  // scores, then the per-partition selection instead of the radix select
    if (m.radix.use_radix) {
        m.defer.can_defer = m.batch.can_batch = false;
        m.defer.fused = false;
        HIP_TRY(m.alloc_ninf_scores(m.radix.d_rscores));  // (m.desc: setup_geometry)
        HIP_TRY(m.alloc(m.radix.d_rhist, 4 * 256 * 4));
    }
    // (every streaming wave of a sequence launch owns ONE partition: an engine packed with more -- the load-only probe's
    //  TKSPMV_PARTITIONS_HINT -- would silently skip the rest)
    if (m.pm.part_first.size() > (size_t)S.n_stream_waves) m.batch.can_batch = m.defer.can_defer = false;
    return TKSPMV_OK;
}

// Multi-query passes (desc.multi_q; TKSPMV_MULTI_Q overrides): a second copy of the matrix in the wave-sliced ELL layout. Ends
// the life of the device packer's COO either way.
static int setup_multi(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    int mq = d.multi_q;
    if (d.impl == TKSPMV_IMPL_ROW_PER_LANE && mq == 0) mq = 1;
    mq = (int)opt_int("MULTI_Q", mq);
    if (mq != 0 && mq != 1 && mq != 2 && mq != 4 && mq != 8) return fail(err, TKSPMV_ERR_INVALID, "multi_q must be 0 (off), 1, 2, 4 or 8");
    // A threshold is the k-th largest of the published group maxima. With k above a quarter of the groups it forms late
    // and stays weak; with 8 queries per pass the private lists are half as long (64 entries) and the held slices
    // fewer: measured at k = 500 (while that kernel still ran one workgroup per CU) every wave ran into its bounded
    // wait and then poured its rows into the overflow list, 2 ms per query. Such engines run 4 queries per pass.
    if (mq == 8 && (uint32_t)d.k * 4u > m.ex.n_groups_pub) mq = 4;
    m.multi.multi_q = mq;
    // One or two queries per pass: a launch makes several passes (MULTI_PASSES; default: as many as the MULTI_Q_MAX queries of
    // a group allow -- 8 or 4), each pass with its own queries and exchange-state sets. (4 and 8 per pass: one pass per launch.)
    m.multi.multi_group = mq;
    if (mq == 1 || mq == 2) {
        m.multi.multi_group = (int)opt_int("MULTI_PASSES", MULTI_Q_MAX / mq, 1, MULTI_Q_MAX / mq) * mq;
    }
    // 8 queries per pass need 91 registers: with 9 waves per workgroup only one workgroup fits a CU (the dispatcher wants
    // 6 waves on one SIMD for two); with 8 waves -- 7 streaming + the server -- two fit at up to 128 registers.
    m.multi.multi_stream_waves = (m.multi.multi_q >= 8 && S.waves_per_wg == 8u) ? 7u : S.waves_per_wg;
    // (k above half of the groups: the threshold is next to useless -- k = 1000 on 1024 groups measured 3.6 ms per query
    // through the multi-query kernel against 0.2 ms one query per pass; such engines keep the ordinary sequence)
    // The selector workgroups of a multi-query launch have multi_stream_waves * 64 + 64 threads and hold SEL_PER_THREAD
    // slots each in registers: every slot of the grid must fit (with 7 streaming waves that is 4096 slots = 512
    // workgroups, fewer than the 576 the ordinary launch geometry allows).
    m.multi.can_multi = mq > 0 && !m.radix.use_radix && m.defer.can_defer && m.ex.n_sets != 0u && d.cols <= SELL_XCOLS &&
                  (d.precision == TKSPMV_F32 || d.precision == TKSPMV_Q1_7_F32) && m.pm.nnz > 0 &&
                  m.grid > 2u * (uint32_t)MULTI_Q_MAX && (uint32_t)d.k * 2u <= m.ex.n_groups_pub &&
                  (uint64_t)m.grid * WG_SLOTS <= (uint64_t)SEL_PER_THREAD * (m.multi.multi_stream_waves * 64u + 64u) &&
                  // (the kernel stages x with TWO words per thread -- multi_kernel's XI --: a workgroup narrower than 512 threads
                  //  would leave the columns from 2 x blockDim on unwritten in LDS and score against garbage, ADVICE r4;
                  //  such geometries -- threads_per_wg <= 384 -- keep the ordinary sequence)
                  2u * (m.multi.multi_stream_waves * 64u + 64u) >= SELL_XCOLS;
    if (m.multi.can_multi) {
        // the first multi_group workgroups of a multi-query launch are its selectors (one per query of the previous launch), the others stream
        const uint32_t n_multi_waves = (m.grid - (uint32_t)m.multi.multi_group) * m.multi.multi_stream_waves;
        SellMatrix sm;
        std::string perr;
        const auto t_sell = std::chrono::steady_clock::now();
        const SellValues sv = d.precision == TKSPMV_Q1_7_F32 ? SellValues::Q1_7_RND : SellValues::F32;
        if (S.prepacked) {  // no COO at hand: decode the packed matrix (byte values decode to exactly representable floats)
            std::vector<uint32_t> r, c;
            std::vector<float> v;
            decode_wbscsr(*S.prepacked, r, c, v);
            perr = pack_wsell(d.rows, d.cols, r.size(), r.data(), c.data(), v.data(), n_multi_waves, sm, sv);
        } else if (S.packed_on_device) {  // plan on the host, fill on the device (device_pack.hip; same bytes)
            DeviceSell ds;
            perr = pack_wsell_device(d.rows, d.cols, d.nnz, d.row, d.col, d.val, n_multi_waves, sv, S.d_coo_col, S.d_coo_val, ds);
            sm = std::move(ds.meta);
            m.multi.d_sell_packets = m.adopt(ds.d_packets);
        } else {
            perr = pack_wsell(d.rows, d.cols, d.nnz, d.row, d.col, d.val, n_multi_waves, sm, sv);
        }
        S.sell_pack_us = (uint32_t)std::min<long long>(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_sell).count(), 0xFFFFFFFFll);
        m.multi.sell_packet_bytes = sm.packet_bytes;
        S.sell_values = sv != SellValues::Q1_7_RND ? 0 : (sm.cw_bits == 12 ? 2 : 1);
        if (!perr.empty()) return fail(err, perr.find("failed:") != std::string::npos ? TKSPMV_ERR_DEVICE : TKSPMV_ERR_INVALID, perr);
        m.multi.sell_parts = (uint32_t)sm.part_first.size();
        S.sell_bytes = sm.stream_bytes() + sm.slice_rows.size() * 4 + (uint64_t)m.multi.sell_parts * 12;
        if (!m.multi.d_sell_packets) {
            HIP_TRY(m.alloc(m.multi.d_sell_packets, std::max<size_t>(sm.stream_bytes(), 256)));
            HIP_TRY(hipMemcpy(m.multi.d_sell_packets, sm.packets.data(), sm.stream_bytes(), hipMemcpyHostToDevice));
        }
        HIP_TRY(m.alloc(m.multi.d_sell_rows, sm.slice_rows.size() * 4));
        HIP_TRY(hipMemcpy(m.multi.d_sell_rows, sm.slice_rows.data(), sm.slice_rows.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(m.alloc(m.multi.d_sell_part_first, (size_t)m.multi.sell_parts * 4));
        HIP_TRY(m.alloc(m.multi.d_sell_part_count, (size_t)m.multi.sell_parts * 4));
        HIP_TRY(m.alloc(m.multi.d_sell_part_slice0, (size_t)m.multi.sell_parts * 4));
        HIP_TRY(hipMemcpy(m.multi.d_sell_part_first, sm.part_first.data(), (size_t)m.multi.sell_parts * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m.multi.d_sell_part_count, sm.part_count.data(), (size_t)m.multi.sell_parts * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m.multi.d_sell_part_slice0, sm.part_slice0.data(), (size_t)m.multi.sell_parts * 4, hipMemcpyHostToDevice));
        HIP_TRY(m.alloc(m.multi.d_multi_out_idx, 2 * (size_t)MULTI_Q_MAX * d.k * 4));
        HIP_TRY(m.alloc(m.multi.d_multi_out_val, 2 * (size_t)MULTI_Q_MAX * d.k * 4));
        HIP_TRY(hipStreamCreateWithFlags(&m.multi.side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&m.multi.ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m.multi.ev_join, hipEventDisableTiming));
        m.multi.multi_chains = opt_int("MULTI_CHAINS", 2) >= 2 ? 2 : 1;
        if (d.stream_replicas > 1) {
            m.multi.d_sell_replicas.push_back(m.multi.d_sell_packets);
            for (int r = 1; r < d.stream_replicas; ++r) {
                uint8_t *p = nullptr;
                HIP_TRY(m.alloc(p, sm.stream_bytes()));
                HIP_TRY(hipMemcpy(p, m.multi.d_sell_packets, sm.stream_bytes(), hipMemcpyDeviceToDevice));
                m.multi.d_sell_replicas.push_back(p);
            }
        }
    }
    m.release(S.d_coo_col);
    m.release(S.d_coo_val);
    return TKSPMV_OK;
}

// The checks of workgroup-local thresholds: the verdict words, the failure estimate that picks the mode, the carried priors and
// their signatures, and the pacing settings.
static int setup_verdicts(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    HIP_TRY(m.alloc(m.batch.d_tickets, BATCH_MAX * 32 * 4, Mem::Exchange, 0));
    HIP_TRY(m.alloc(m.trust.d_verdict, 512, Mem::Exchange, 0));
    // the host's side of the verdicts (EngineImpl::settle); without it every local launch keeps its repair launch in the stream
    if (const char *f = opt("REPAIR")) m.trust.repair_by_host = std::string(f) != "stream";
    if (m.alloc(m.trust.h_verdict, (size_t)EngineImpl::Trust::VERDICT_RING * 8, Mem::Pinned, 0) != hipSuccess ||
        hipHostGetDevicePointer((void **)&m.trust.h_verdict_dev, m.trust.h_verdict, 0) != hipSuccess) {
        m.release(m.trust.h_verdict);
        m.trust.h_verdict = m.trust.h_verdict_dev = nullptr;
        (void)hipGetLastError();
    }
    // Workgroup-local thresholds pay when they practically never fail the selection's check (a failure costs the query a
    // second pass). The workgroup's threshold is the smallest of its waves' words; it exceeds the k-th best score when EVERY
    // streaming wave's word does (a = waves with a partition per workgroup, at least). A wave's word is its best packet
    // maximum (mode 1: lambda = k / partitions of the k best rows sit in a wave: ~lambda) or its second best (mode 2: two of
    // them in different packets, ~lambda^2 / 2; a single-packet partition has no second one). Mode 1 forms the threshold a
    // packet earlier: preferred where it is safe. And a workgroup keeps its 8 best rows: 9 of the k best in one workgroup
    // fail too (Poisson tail at k / workgroups).
    const double n_parts = (double)std::max<size_t>(m.pm.part_first.size(), 1), n_wg = (double)(m.grid - m.batch.n_sel_wg);
    const double lam = std::min(1.0, (double)d.k / n_parts);
    const double per_part = (double)m.pm.n_packets / n_parts;
    const double a = std::max(1.0, std::floor(n_parts / n_wg));
    const double lw = (double)d.k / n_wg;
    double tail9 = 1.0, term = std::exp(-lw);
    for (int i = 0; i < 9; ++i) { tail9 -= term; term *= lw / (i + 1); }
    tail9 = std::max(tail9, 0.0);
    const double p1 = n_wg * (std::pow(lam, a) + tail9);
    const double p2 = n_wg * (std::pow(per_part < 1.5 ? lam : std::min(1.0, 0.5 * lam * lam), a) + tail9);
    m.local.single_mode = m.grid > 512u ? 0u : (p1 <= 1e-4 ? 1u : (p2 <= 1e-3 ? 2u : 0u));  // (512: select_local's record count)
    // Back-to-back queries: beyond ~1.3M rows the device-wide exchange is as fast and checks nothing (small_matrix). ONE query per
    // launch has no such cross-over -- without a previous query in flight the exchange's threshold arrives a third into the
    // partition, a carried local one is there from the first packet: 58.4 against 67.5 us at 3M rows -- so single_kernel serves
    // tkspmv_run wherever the failure estimate allows it.
    m.local.use_local = S.small_matrix ? m.local.single_mode : 0u;
    if (opt("DEBUG_OCC"))
        fprintf(stderr, "[tkspmv] small matrix %d: %u selector workgroups, %.0f partitions of %.1f packets, %.0f per workgroup; local thresholds fail with p = %.2e (mode 1) / %.2e (mode 2): mode %u\n",
                (int)S.small_matrix, m.batch.n_sel_wg, n_parts, per_part, a, p1, p2, m.local.use_local);
    HIP_TRY(m.alloc(m.local.d_wg_prior, ((size_t)m.grid + 32) * 4, Mem::Exchange, 0));  // priors | countdown words
    if (opt_int("SIGNATURES", 1) != 0) HIP_TRY(m.alloc(m.local.d_wg_sig, (size_t)m.grid * 8 * 4, Mem::Device, 0));
    if (const char *f = opt("LOCAL_BETA")) m.local.local_beta = (float)atof(f);
    if (opt_set("LOCAL")) m.local.use_local = m.local.single_mode = m.grid > 512u ? 0u : (uint32_t)opt_int("LOCAL", 0, 0, 2);
    // Pacing by rank, with local thresholds only (with the device-wide exchange the cold phase of every query is governor enough, §3.0):
    // the longer the partitions, the longer the pause (size sweeps on two boxes, tools/ab_rank.sh: best at 0 / 1 / 2 units of 256 cycles
    // up to 575k / 830k / 1.3M rows of 20 non-zeros).
    // The pause follows the packet's size (fp32 values with 12-bit columns, 1408 bytes: 2 units; fp16, 896 bytes: 1 -- 15.4 us per query
    // at 1M rows against 16.3 at 2 units and 16.7 with the device-wide exchange).
    // (units of 128 cycles per level)
    // (the canonical packet's size is read here, ahead of compact_stream: the compact fp32 packets, 1280 bytes, round to the same 2 units)
    // (round 5, with the pause behind the packet's arithmetic: from ~330k rows up a pause of ONE unit per level pays -- 500k rows: 9.03
    //  against 9.86 us per query unpaced, 10.0 at two units; 250k rows: 5.8 either way -- and tkspmv_create's measurement may still
    //  choose none)
    if (m.local.use_local) m.local.pace_quads = m.pm.n_packets <= 25000u ? 0u : (m.pm.n_packets <= 45000u ? 1u : (m.pm.n_packets <= 65000u ? 2u : 2u * std::max(1u, (m.pm.packet_bytes + 352u) / 704u)));
    m.local.pace_levels = (uint32_t)opt_int("PACE_LEVELS", m.local.pace_levels, 1, 8);
    m.local.pace_quads = (uint32_t)opt_int("PACE", m.local.pace_quads, 0, 32);
    m.local.pace_base = (uint32_t)opt_int("PACE_BASE", 0, 0, 64);
    m.local.pace_carry = opt_int("PACE_CARRY", 1) != 0;
    m.local.pace_adapt_on = opt_int("PACE_ADAPT", 1) != 0;
    m.local.pace_period_ns = (uint32_t)opt_int("PACE_PERIOD", 0, 0, 10000000);
    m.range.range_period_set = opt_set("RANGE_PERIOD");
    m.range.range_period_ns = (uint32_t)opt_int("RANGE_PERIOD", 0, 0, 10000000);
    const long facet_cap = (long)facet_lds_bins(m.fmt.xcols);
    m.range.facet_lds_bins = (uint32_t)opt_int("FACET_LDS_BINS", facet_cap, 0, facet_cap);
    if (m.local.use_local && m.local.pace_quads != 0u) {
        HIP_TRY(m.alloc(m.local.d_wg_pace, (size_t)m.grid * 4, Mem::Device, 0));
        HIP_TRY(m.alloc(m.local.d_pace_adapt, 128, Mem::Exchange, 0));
    }
    return TKSPMV_OK;
}

// single_kernel serves tkspmv_run where the engine streams with local thresholds: a format it is built for (has_single_kernel),
// at most 512 workgroups (select_local's first cut), one partition per wave of ITS launch (8 waves x grid).
static int setup_single(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    m.single.can_single = m.local.single_mode != 0u && has_single_kernel(m.fmt) && m.grid <= 512u && m.block == 512u &&
                   d.impl == TKSPMV_IMPL_STREAM && !m.radix.use_radix && m.defer.fused && m.host.host_path && m.host.h_res != nullptr &&
                   m.pm.part_first.size() <= (size_t)m.grid * 8u;
    m.single.can_single = m.single.can_single && opt_int("SINGLE", 1) != 0;
    if (!m.single.can_single) return TKSPMV_OK;
    HIP_TRY(m.alloc(m.single.d_lslots, (size_t)m.grid * SINGLE_REC_STRIDE * 8, Mem::Device, 0xFF));  // (a 128-byte line per workgroup: single_kernel's selector)
    // workgroup 0 selects (LocalParams::ready) where the partitions fit the grid's other workgroups; option SINGLE_SELECTOR=0:
    // round 4's scheme (every workgroup streams, the one that draws the last ticket selects)
    if (m.pm.part_first.size() <= (size_t)(m.grid - 1u) * 8u && m.grid >= 2u && opt_int("SINGLE_SELECTOR", 1) != 0)
        HIP_TRY(m.alloc(m.single.d_lready, (size_t)m.grid * 4, Mem::Exchange, 0));
    HIP_TRY(m.alloc(m.single.d_lused, (size_t)m.grid * 4, Mem::Device, 0));
    HIP_TRY(m.alloc(m.single.d_lprior, ((size_t)m.grid + 32) * 4, Mem::Exchange, 0));
    HIP_TRY(m.alloc(m.single.d_lstatus, 128, Mem::Exchange, 0));
    return TKSPMV_OK;
}

// Exchange-state sets: one block per field, set s at s strides (the batch kernel addresses them that way). The batch kernel
// runs one set per query of a launch; every set is small -- published maxima, a threshold word, one slot per wave --
// except for the overflow list, which must be able to hold EVERY row (a degenerate query -- x = 0, all scores equal --
// makes every row a candidate and the result must still be exact): 8 bytes per row. Round 3 kept one list per set: 256 MB
// at 1M rows, 2.6 GB at 10M. Engines of the batch kernel now keep FOUR, which the queries of a launch share round robin
// under flow control (BatchParams::ovf_epoch), and the general path of the selection needs no scratch copy any more
// (select_body): 32 MB at 1M rows, 320 MB at 10M. Multi-query engines keep one list per set (their groups' selections are
// owed across launches).
static int setup_exchange_sets(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    using Sets = EngineImpl::ExchangeSets;
    m.batch.batch_max = (int)opt_int("BATCH_MAX", BATCH_MAX, 1, BATCH_MAX);
    const int n_sets_alloc = m.multi.can_multi ? Sets::N_STATE : (m.batch.can_batch ? m.batch.batch_max : (m.defer.can_defer ? 2 : 1));
    const size_t ns = (size_t)n_sets_alloc;
    // (engines that stream with checked local thresholds use the lists for repairs and behind a closed gate only: two; a power of two)
    int want_lists = (int)opt_int("OVF_LISTS", m.local.use_local ? 2 : 4);
    // (the deferred scheme streams query i + 1 into one set while workgroup 0 selects query i from the other: its two sets need
    //  private lists -- with OVF_LISTS=1 they shared one, the stream appended while the selection read and reset it)
    if (m.defer.can_defer) want_lists = std::max(want_lists, 2);
    want_lists = std::min(std::min(want_lists, 4), n_sets_alloc);
    m.ex.ovf_lists = m.multi.can_multi ? (uint32_t)n_sets_alloc : (want_lists >= 4 ? 4u : (want_lists >= 2 ? 2u : 1u));
    const size_t nl = m.ex.ovf_lists;
    Sets::ExState &E0 = m.ex.st[0];  // (the other sets point into its blocks)
    HIP_TRY(m.alloc(E0.gmax, ns * Sets::GMAX_WORDS * 4, Mem::Exchange, 0));
    HIP_TRY(m.alloc(E0.tau_g, ns * Sets::STATE_WORD_STRIDE * 4, Mem::Exchange, 0));
    HIP_TRY(m.alloc(E0.ovf_count, nl * Sets::STATE_WORD_STRIDE * 4, Mem::Device, 0));
    HIP_TRY(m.alloc(E0.wg_cand, ns * m.grid * WG_SLOTS * 8, Mem::Device, 0xFF));
    HIP_TRY(m.alloc(E0.ovf, nl * m.ex.ovf_cap * 8));
    const size_t n_unit = std::max(ns, (size_t)BATCH_MAX);  // (the batch kernel's scale words)
    HIP_TRY(m.alloc(E0.unit_inv, n_unit * Sets::STATE_WORD_STRIDE * 4));
    std::vector<float> ones(n_unit * Sets::STATE_WORD_STRIDE, 1.0f);
    HIP_TRY(hipMemcpy(E0.unit_inv, ones.data(), ones.size() * 4, hipMemcpyHostToDevice));
    for (int si = 1; si < n_sets_alloc; ++si) {
        Sets::ExState &E = m.ex.st[si];
        E.gmax = E0.gmax + (size_t)si * Sets::GMAX_WORDS;
        E.tau_g = E0.tau_g + (size_t)si * Sets::STATE_WORD_STRIDE;
        E.ovf_count = E0.ovf_count + ((size_t)si % nl) * Sets::STATE_WORD_STRIDE;
        E.wg_cand = E0.wg_cand + (size_t)si * m.grid * WG_SLOTS;
        E.ovf = E0.ovf + ((size_t)si % nl) * m.ex.ovf_cap;
        E.unit_inv = E0.unit_inv + (size_t)si * Sets::STATE_WORD_STRIDE;
    }
    HIP_TRY(m.alloc(m.ex.d_ovf_epoch, 128, Mem::Exchange, 0));
    if (m.batch.can_batch) {
        // the workgroups' records of local mode, one block per set; the scratch results of queries that share the last one's buffer
        const size_t nr = (size_t)BATCH_MAX;
        HIP_TRY(m.alloc(m.batch.d_rec_slots, nr * m.grid * WG_SLOTS * 8, Mem::Device, 0xFF));
        HIP_TRY(m.alloc(m.batch.d_rec_used, nr * m.grid * 4, Mem::Device, 0));
        HIP_TRY(m.alloc(m.batch.d_alias_idx, nr * d.k * 4));
        HIP_TRY(m.alloc(m.batch.d_alias_val, nr * d.k * 4));
    }
    m.info.state_bytes = ns * (Sets::GMAX_WORDS * 4 + 2 * Sets::STATE_WORD_STRIDE * 4 + (uint64_t)m.grid * WG_SLOTS * 8) +
                         nl * ((uint64_t)m.ex.ovf_cap * 8 + Sets::STATE_WORD_STRIDE * 4) +
                         (m.batch.can_batch ? (uint64_t)BATCH_MAX * ((uint64_t)m.grid * WG_SLOTS * 8 + (uint64_t)m.grid * 4) : 0);
    return TKSPMV_OK;
}

// The buffers of the tracing and statistics options and the DEBUG_OCC occupancy report.
static int setup_diagnostics(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    m.diag.collect_stamps = opt("STAMPS") != nullptr;
    if (opt("WG_TIMES") && m.local.use_local) HIP_TRY(m.alloc(m.diag.d_wg_times, (size_t)(BATCH_MAX + 1) * m.grid * 8, Mem::Device, 0));
    if (opt("TRACE")) {
        m.diag.trace_words = (size_t)(m.grid + 1) * 9 * 8;
        HIP_TRY(m.alloc(m.diag.d_trace, m.diag.trace_words * 4 * 8, Mem::Device, 0));
    }
    m.diag.dbg_kernels = m.diag.collect_stats || m.diag.collect_stamps || m.diag.d_trace != nullptr;
    if (m.diag.dbg_kernels && !has_tracing_twins(m.fmt))
        fprintf(stderr, "[tkspmv] tracing / statistics hooks exist in the fp32, 4-entries-per-lane, <= 1024-column kernels only: "
                        "this engine runs without them\n");
    return TKSPMV_OK;
}

// ---- the batch kernel's compact copies (wbscsr.hpp F32E5) ---------------------------------------------------------------------
// The census of a resident F32C12 stream (f32e5_census_entry over every entry): one thread per lane of a packet, a wave's share
// reduced in registers, four atomics per wave. out: [0] AND, [1] OR of the words that are not +0.0, [2..3] the bare zeros (64 bits),
// [4] the odd SKIPs.
__global__ void __launch_bounds__(256) f32e5_census_kernel(const uint8_t *__restrict__ packets, uint32_t n_packets, uint32_t packet_bytes, uint32_t *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = (uint32_t)(t & 63u);
    uint32_t a = 0xFFFFFFFFu, o = 0u, bare = 0u, odd = 0u;
    if (t / 64u < n_packets) {  // (whole waves: a packet is a wave's)
        const uint8_t *pkt = packets + (size_t)(t / 64u) * packet_bytes;
        for (uint32_t j = 0; j < 4u; ++j) {
            uint32_t bz, os;
            f32e5_census_entry(get<uint32_t>(pkt + (size_t)(lane * 4u + j) * 4), colw12s_load(pkt + (size_t)F32E5_PACKET_ENTRIES * 4, lane * 4u + j), a, o, bz, os);
            bare += bz;
            odd += os;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        a &= (uint32_t)__shfl_xor((int)a, d);
        o |= (uint32_t)__shfl_xor((int)o, d);
        bare += (uint32_t)__shfl_xor((int)bare, d);
        odd += (uint32_t)__shfl_xor((int)odd, d);
    }
    if (lane == 0u) {
        if (a != 0xFFFFFFFFu) atomicAnd(out + 0, a);
        if (o != 0u) atomicOr(out + 1, o);
        if (bare != 0u) atomicAdd(reinterpret_cast<unsigned long long *>(out + 2), (unsigned long long)bare);
        if (odd != 0u) atomicAdd(out + 4, odd);
    }
}
// The re-encoding, packet for packet: thread t = lane t % 64 of packet t / 64 (f32e5_transcode_lane, the host re-encoder's function).
__global__ void __launch_bounds__(256) f32e5_transcode_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t n_packets, uint32_t packet_bytes) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t / 64u >= n_packets) return;
    f32e5_transcode_lane(src + (size_t)(t / 64u) * packet_bytes, dst + (size_t)(t / 64u) * F32E5_PACKET_BYTES, (uint32_t)(t & 63u));
}

// Engines whose batch kernel reads an F32C12 stream get compact copies of it where the matrix's values allow (option F32_COMPACT=0:
// never): a device reduction decides (all fp32 words share their top four bits; no +0.0 but placeholders and padding), a device
// kernel re-encodes the stream into as many copies as the canonical stream has. Entry order, partitions, pkt_row and the tables stay
// what they are, so does the arithmetic: the results are the canonical stream's bit for bit. Engines that trace stay on F32C12 (the
// new format has no tracing twin). Behind setup_diagnostics (who traces?), ahead of choose_kernels.
static int compact_stream(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    if (opt_int("F32_COMPACT", 1) == 0 || !m.batch.can_batch || m.diag.dbg_kernels || m.fmt.qm != QM_F32C12 || !f32e5_applies(m.pm) || !m.mat.d_packets)
        return TKSPMV_OK;
    ScratchBuffer<uint32_t> census;
    HIP_TRY(hipMalloc((void **)&census.p, 32));
    const uint32_t init[8] = {0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    HIP_TRY(hipMemcpy(census.p, init, sizeof(init), hipMemcpyHostToDevice));
    const uint32_t blocks = (uint32_t)(((uint64_t)m.pm.n_packets * 64u + 255u) / 256u);
    hipLaunchKernelGGL(f32e5_census_kernel, dim3(blocks), dim3(256), 0, m.stream, m.mat.d_packets, m.pm.n_packets, m.pm.packet_bytes, census.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m.stream));
    uint32_t got[8];
    HIP_TRY(hipMemcpy(got, census.p, sizeof(got), hipMemcpyDeviceToHost));
    F32E5Census c;
    c.all_and = got[0];
    c.all_or = got[1];
    c.bare_zeros = (uint64_t)got[2] | ((uint64_t)got[3] << 32);
    c.odd_skips = got[4];
    uint32_t top4 = 0u;
    if (!f32e5_census_eligible(c, f32e5_padding(m.pm), top4)) return TKSPMV_OK;  // signed, zero-bearing or wide-ranged values: the engine runs as it is
    const size_t bytes = (size_t)m.pm.n_packets * F32E5_PACKET_BYTES;
    const size_t copies = std::max<size_t>(m.mat.d_replicas.size(), 1);
    for (size_t r = 0; r < copies; ++r) {
        uint8_t *p = nullptr;
        if (m.alloc(p, bytes) != hipSuccess) {  // no room for a second set of copies: the engine streams the canonical ones
            (void)hipGetLastError();
            for (uint8_t *q : m.mat.d_compact) m.release(q);
            m.mat.d_compact.clear();
            return TKSPMV_OK;
        }
        if (r == 0) {
            hipLaunchKernelGGL(f32e5_transcode_kernel, dim3(blocks), dim3(256), 0, m.stream, m.mat.d_packets, p, m.pm.n_packets, m.pm.packet_bytes);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(m.stream));
        } else {
            HIP_TRY(hipMemcpy(p, m.mat.d_compact[0], bytes, hipMemcpyDeviceToDevice));
        }
        m.mat.d_compact.push_back(p);
    }
    m.mat.compact_top4 = top4;
    return TKSPMV_OK;
}

// The kernels of this engine's format (behind setup_diagnostics: an engine that traces takes the tracing twins), and the DEBUG_OCC
// occupancy report about them.
static int choose_kernels(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    m.kern = kernels_for(m.fmt, m.diag.dbg_kernels);
    if (m.mat.compact()) {  // the batch path streams the compact copies (compact_stream): local thresholds, the exact kernel, both repair modes
        m.kern.batch[0] = &batch_kernel<4, 1024, QM_F32E5, false, false>;
        m.kern.batch[1] = &batch_kernel<4, 1024, QM_F32E5, false, true>;
    }
    if (m.multi.can_multi) {  // [value type of the row-per-lane copy][queries per pass: 1, 2, 4, 8]
        static const multi_fn fns[3][4] = {{&multi_kernel<1, VT_F32>, &multi_kernel<2, VT_F32>, &multi_kernel<4, VT_F32>, &multi_kernel<8, VT_F32>},
                                           {&multi_kernel<1, VT_Q17>, &multi_kernel<2, VT_Q17>, &multi_kernel<4, VT_Q17>, &multi_kernel<8, VT_Q17>},
                                           {&multi_kernel<1, VT_Q17C12>, &multi_kernel<2, VT_Q17C12>, &multi_kernel<4, VT_Q17C12>, &multi_kernel<8, VT_Q17C12>}};
        const int q = m.multi.multi_q;
        m.kern.multi = fns[S.sell_values][q <= 1 ? 0 : (q <= 2 ? 1 : (q <= 4 ? 2 : 3))];
    }
    if (opt("DEBUG_OCC")) {
        int n1 = -1, n2 = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1, reinterpret_cast<const void *>(m.kern.stream[0]), (int)m.block + 64, 0);
        if (m.batch.can_batch)
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n2, reinterpret_cast<const void *>(m.kern.batch[0]), (int)m.block + 64, 0);
        fprintf(stderr, "[tkspmv] workgroups per CU by the runtime's occupancy calculator: stream kernel %d, batch kernel %d; LDS per CU %zu\n",
                n1, n2, S.lds_per_cu);
    }
    return TKSPMV_OK;
}

// tkspmv_info: what fill_info could not know at packing time.
static int fill_engine_info(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &) {
    m.info.precision = d.precision;  // the API's enum (fill_info reports the value type of the stream)
    m.info.grid = m.grid;
    m.info.block = m.block;
    m.info.n_groups = m.ex.n_sets ? m.ex.n_groups_pub : 0;
    m.info.lds_bytes = m.ex.lds_bytes;
    m.info.partitions = d.partitions > 1 ? d.partitions : 1;
    m.info.k_per_partition = d.k_per_partition > 0 ? d.k_per_partition : d.k;
    m.info.device = m.device;
    m.info.num_cus = S.num_cus;
    m.info.multi_q = m.multi.can_multi ? (uint32_t)m.multi.multi_q : 0u;
    m.info.multi_bytes = m.multi.can_multi ? S.sell_bytes : 0u;
    m.info.pack_us = S.pack_us;
    m.info.multi_pack_us = S.sell_pack_us;
    m.info.pack_on_device = S.packed_on_device ? 1u : 0u;
    m.info.claim_sets = 0u;
    m.info.batch_compact = m.mat.compact() ? 1u : 0u;
    m.info.batch_packet_bytes = m.mat.batch_packet_bytes(m.pm);
    m.info.batch_stream_bytes = (uint64_t)m.pm.n_packets * m.info.batch_packet_bytes;
    m.info.batch_mode = (m.batch.can_batch ? (m.batch.n_sel_wg | (m.local.use_local << 8)) : 0u) | (std::min<uint32_t>(S.n_parts_hint, 0xFFFFu) << 16);
    return TKSPMV_OK;
}

// Pointer lists of a back-to-back sequence: query i = dev_xs + (i % n_x) * cols; its result goes to dev_idx / dev_val + i * k, or,
// where none are given, into the engine's own pair (every query: the last one wins).
struct SequenceLists {
    std::vector<const float *> xs;
    std::vector<uint32_t *> oi;
    std::vector<float *> ov;
    SequenceLists(const EngineImpl &m, const float *dev_xs, int32_t n_x, int32_t count, uint32_t *dev_idx = nullptr, float *dev_val = nullptr)
        : xs(count), oi(count), ov(count) {
        const size_t stride = dev_idx ? (size_t)m.desc.k : 0;
        for (int i = 0; i < count; ++i) {
            xs[i] = dev_xs + (size_t)(i % n_x) * m.desc.cols;
            oi[i] = (dev_idx ? dev_idx : m.host.d_out_idx) + (size_t)i * stride;
            ov[i] = (dev_val ? dev_val : m.host.d_out_val) + (size_t)i * stride;
        }
    }
};

// ---- pacing, tuned on THIS box for THIS matrix (round 5) ----------------------------------------------------------------------
// The pause per packet of the workgroups that lead the field (BatchParams::pace_quads x pace_levels) decides whether the eight
// XCDs share the memory system evenly -- unpaced, four of them stream a query in 12 us and the other four in 22-26
// (tools/wg_times.py) -- and its best setting moves with the box: quantum 2 over 6 eighths on the pool's fast boxes (16.3 us per
// query, 17.6 at round 4's 4 over 3), 2 over 7 on its slow ones (17.4 against 18.9 and 20.0). So the engine measures: a handful of
// settings, three launches of 32 synthetic queries each, twice through, behind 64 launches of warm-up (tune_rank_pauses); then
// the period of a timetable (tune_timetable): ~140 ms of tkspmv_create at 1M rows.
static const uint32_t PACE_CANDIDATES[][2] = {{2, 6}, {2, 7}, {3, 5}, {4, 4}, {2, 5}, {4, 3}, {1, 6}, {1, 4}, {0, 3}};  // ({0, .}: unpaced)
constexpr int N_PACE_CANDIDATES = (int)(sizeof(PACE_CANDIDATES) / sizeof(PACE_CANDIDATES[0]));

// The measurement's synthetic queries: one launch of the batch kernel on the engine's stream.
static void tune_launch(EngineImpl &m, const SequenceLists &Q) { m.launch_batch(Q.xs.data(), Q.oi.data(), Q.ov.data(), (int)Q.xs.size(), m.stream); }

// Pauses by rank: ms per two launches of every candidate (the better of two passes); leaves the best one in m.
static int tune_rank_pauses(EngineImpl &m, const SequenceLists &Q, float (&best_ms)[N_PACE_CANDIDATES], int &best, std::string &err) {
    for (float &b : best_ms) b = 1e30f;
    // (a GPU that has idled streams 10-15 % slower for its first ~20 ms -- 19.4 us per query falling to 16.7 over thirty launches,
    //  tools/launch_series.py --: the settings are compared on a GPU that has been busy for 64 launches)
    m.local.pace_quads = PACE_CANDIDATES[0][0];
    m.local.pace_levels = PACE_CANDIDATES[0][1];
    for (int w = 0; w < 64; ++w) tune_launch(m, Q);
    if (const int st = m.wait_idle(err)) return st;
    for (int pass = 0; pass < 2; ++pass)
        for (int c = 0; c < N_PACE_CANDIDATES; ++c) {
            m.local.pace_quads = PACE_CANDIDATES[c][0];
            m.local.pace_levels = PACE_CANDIDATES[c][1];
            tune_launch(m, Q);  // (settles the pauses the setting leads to)
            float ms = 0;
            if (const int st = m.bracket_ms(ms, err, [&] { tune_launch(m, Q); tune_launch(m, Q); })) return st;
            HIP_TRY(m.settle());
            best_ms[c] = std::min(best_ms[c], ms);
        }
    best = 0;
    for (int c = 1; c < N_PACE_CANDIDATES; ++c)
        if (best_ms[c] < best_ms[best]) best = c;
    m.local.pace_quads = PACE_CANDIDATES[best][0];
    m.local.pace_levels = PACE_CANDIDATES[best][1];
    return TKSPMV_OK;
}

// The timetable (pacing by the clock, BatchParams::pace_period). Its period must be what THIS box sustains with THIS kernel: a per
// cent too short and the waves fall behind, nobody pauses and the XCDs are back to sharing unevenly (+5 %); too long costs what it
// is too long by. The best period sits 5-6 % under the time per query of the pauses by rank just measured (rank_ms per two launches;
// 15.8 us on the pool's fast boxes, 16.0 on a medium one): a coarse grid around that, then half a per cent either side of its best;
// kept in m.pace_period_ns only if it beats the pauses by rank. Returns the fine search's best period and its ms per two launches.
static uint32_t tune_timetable(EngineImpl &m, const SequenceLists &Q, float rank_ms, float &period_ms) {
    // (ms per TWO launches, the mean over `launches` of them in one go, the better of `passes` such series)
    // (a HIP call that fails leaves `measure_failed` set: the timetable is then not taken, the pauses by rank stay)
    bool measure_failed = false;
    auto measure = [&](uint32_t ns, int passes, int launches) -> float {
        m.local.pace_period_ns = ns;
        float b = 1e30f;
        for (int pass = 0; pass < passes; ++pass) {
            tune_launch(m, Q);
            float ms = 0;
            std::string why;
            const bool ok = m.bracket_ms(ms, why, [&] { for (int l = 0; l < launches; ++l) tune_launch(m, Q); }) == TKSPMV_OK &&
                            m.wait_idle(why) == TKSPMV_OK && hipGetLastError() == hipSuccess;
            if (!ok) {
                measure_failed = true;
                return 1e30f;
            }
            b = std::min(b, ms * 2.0f / (float)launches);
        }
        return b;
    };
    period_ms = 1e30f;
    uint32_t period_ns = 0;
    const double rank_ns = (double)rank_ms * 1e6 / (2.0 * (double)Q.xs.size());  // per query
    static const double grid[] = {0.90, 0.915, 0.93, 0.945, 0.96, 0.975};
    for (double g : grid) {
        const uint32_t ns = (uint32_t)(rank_ns * g);
        const float ms = measure(ns, 2, 2);
        if (ms < period_ms) {
            period_ms = ms;
            period_ns = ns;
        }
    }
    // The grid's best is the best of single launches. Back to back, a period that close to what the kernel sustains has
    // every fourth launch or so run 8-10 % longer (for ~100 us the memory system gives less, one XCD's workgroups take the whole
    // shortfall, fall 40-80 us behind and the launch waits for them: tools/spike_probe.py); 2 % more period and those launches
    // are gone (same box: 16.7 us per query with spikes to 18.5 at 15.8 us, 16.9 without any at 16.1). So the fine search
    // measures series of eight launches -- their mean --, from the grid's best upwards.
    const uint32_t centre = period_ns;
    period_ms = 1e30f;
    for (double g : {1.03, 1.02, 1.01, 1.0, 0.99}) {
        const uint32_t ns = (uint32_t)((double)centre * g);
        const float ms = measure(ns, 2, 8);
        // (from the longest period down: a shorter one must measure 0.3 % better to be taken -- a single launch at a period
        //  close to what the kernel sustains runs 4-5 % long one time in eight, which a mean over eight launches half hides)
        if (ms < period_ms * 0.997f) {
            period_ms = ms;
            period_ns = ns;
        }
    }
    m.local.pace_period_ns = (!measure_failed && period_ms < rank_ms * 0.999f) ? period_ns : 0u;
    return period_ns;
}

// Engines of checked local thresholds that pace at all (every packet size since the pause sits behind the arithmetic: fp16 and the
// fixed-point streams gain as fp32 does); options PACE / PACE_LEVELS / PACE_BASE / AUTOTUNE=0 keep the static settings.
static int autotune_pacing(const tkspmv_desc &d, Setup &S, EngineImpl &m, std::string &err) {
    if (!(m.local.use_local && m.batch.can_batch && m.local.pace_quads != 0u && !opt("PACE") && !opt("PACE_LEVELS") && !opt("PACE_BASE") &&
          opt_int("AUTOTUNE", 1) != 0))
        return TKSPMV_OK;
    // (launches of 32 queries up to the headline's size; fewer queries per launch on larger matrices, so that the measurement stays
    //  at ~150 ms of streaming: 10M rows -- 5.3 ms per launch of 32 -- would spend 1.3 s on it)
    const int nq = std::max(4, std::min(std::min((int)BATCH_MAX, m.batch.batch_max), (int)(32ull * 80000ull / std::max<uint64_t>(m.pm.n_packets, 1))));
    std::vector<float> hx((size_t)nq * d.cols);
    uint32_t lcg = 0x1234567u;
    for (float &v : hx) {
        lcg = lcg * 1664525u + 1013904223u;
        v = (float)(lcg >> 8) * (1.0f / 16777216.0f);
    }
    ScratchBuffer<float> tx;
    HIP_TRY(hipMalloc((void **)&tx.p, hx.size() * 4));
    HIP_TRY(hipMemcpy(tx.p, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
    const SequenceLists Q(m, tx.p, nq, nq);  // (into the engine's own result pair)
    const auto t_tune = std::chrono::steady_clock::now();
    const bool adapt_was = m.local.pace_adapt_on;
    m.local.pace_adapt_on = false;  // (the periods are measured as they are given)
    float best_ms[N_PACE_CANDIDATES];
    int best = 0;
    if (const int st = tune_rank_pauses(m, Q, best_ms, best, err)) return st;
    float period_ms = 1e30f;
    uint32_t period_ns = 0;
    if (!opt("PACE_PERIOD")) period_ns = tune_timetable(m, Q, best_ms[best], period_ms);
    const uint32_t tune_us = (uint32_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_tune).count();
    // the engine starts as if nothing had run: no carried thresholds, no pauses, no counters, no trust
    HIP_TRY(hipMemset(m.local.d_wg_prior, 0, ((size_t)m.grid + 32) * 4));
    if (m.local.d_wg_pace) HIP_TRY(hipMemset(m.local.d_wg_pace, 0, (size_t)m.grid * 4));
    if (m.local.d_wg_sig) HIP_TRY(hipMemset(m.local.d_wg_sig, 0, (size_t)m.grid * 8 * 4));
    m.trust.clean_seen = m.trust.distrust_left = 0u;
    m.trust.trusted_launches = m.trust.late_repairs = 0;
    m.local.pace_tune_launches = (uint32_t)m.batch.batch_launches;
    m.batch.batch_launches = 0;
    HIP_TRY(hipMemset(m.trust.d_verdict, 0, 512));
    HIP_TRY(hipMemset(m.host.d_out_idx, 0, (size_t)d.k * 4));
    HIP_TRY(hipMemset(m.host.d_out_val, 0, (size_t)d.k * 4));
    m.local.pace_tuned_us = tune_us ? tune_us : 1u;
    m.local.pace_adapt_on = adapt_was;
    if (opt("DEBUG_OCC")) {
        fprintf(stderr, "[tkspmv] pacing tuned in %u us:", tune_us);
        for (int c = 0; c < N_PACE_CANDIDATES; ++c)
            fprintf(stderr, " %ux%u %.2f us/q%s", PACE_CANDIDATES[c][0], PACE_CANDIDATES[c][1], best_ms[c] * 1e3 / (2 * nq), c == best ? "*" : "");
        fprintf(stderr, "; timetable %u ns: %.2f us/q%s\n", period_ns, period_ms * 1e3 / (2 * nq), m.local.pace_period_ns ? " (kept)" : " (pauses by rank kept)");
    }
    return TKSPMV_OK;
}

static int create_impl(const tkspmv_desc &d, EngineImpl &m, std::string &err, const PackedMatrix *prepacked = nullptr) {
    // (in this order: the descriptor is checked before any device call, and the HIP calls keep one sequence)
    static int (*const stages[])(const tkspmv_desc &, Setup &, EngineImpl &, std::string &) = {
        check_desc,  setup_geometry, pack_matrix,    exchange_geometry,   upload_matrix,     setup_host_boundary, choose_path,
        setup_multi, setup_verdicts, setup_single, setup_exchange_sets, setup_diagnostics, compact_stream,      choose_kernels,      fill_engine_info,
        autotune_pacing};
    Setup S{prepacked};
    for (auto stage : stages)
        if (const int st = stage(d, S, m, err)) return st;
    HIP_TRY(hipDeviceSynchronize());
    return TKSPMV_OK;
}

Engine *Engine::create(const tkspmv_desc &desc, std::string &err, int &status, const PackedMatrix *prepacked) {
    Engine *e = new Engine();
    e->impl_ = new EngineImpl();
    status = create_impl(desc, *e->impl_, err, prepacked);
    if (status != TKSPMV_OK) {
        delete e;
        return nullptr;
    }
    return e;
}

void Engine::info(tkspmv_info *out) const { *out = impl_->info; }

int wave_partitions_for(const tkspmv_desc &d, uint32_t *out, std::string &err) {
    int dev = d.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    const uint32_t block = d.threads_per_wg > 0 ? (uint32_t)d.threads_per_wg : 512u;
    const uint32_t waves_per_cu = d.waves_per_cu > 0 ? (uint32_t)d.waves_per_cu : 16u;
    const uint32_t waves_per_wg = block / 64;
    const uint32_t grid = std::max(1u, (uint32_t)prop.multiProcessorCount * waves_per_cu / waves_per_wg);
    const bool defer_capable = grid >= 2 && (uint64_t)grid * WG_SLOTS <= (uint64_t)SEL_PER_THREAD * (block + 64);
    // (with the matrix described -- rows, cols, nnz, precision --: the hint tkspmv_create itself would pack this matrix with;
    //  without: the largest count any engine of this geometry accepts)
    *out = (grid - (defer_capable ? small_matrix_settings(d, grid, defer_capable, entries_per_lane_of(d), nullptr) : 0u)) * waves_per_wg;
    return TKSPMV_OK;
}

int Engine::set_query(const float *host_x, double *elapsed_ns, std::string &err) {
    EngineImpl &m = *impl_;
    if (!host_x) return fail(err, TKSPMV_ERR_INVALID, "query vector is NULL");
    auto t0 = std::chrono::high_resolution_clock::now();
    HIP_TRY(hipSetDevice(m.device));
    if (m.host.bar_x) {
        // (a launch enqueued earlier may still be reading d_x: tkspmv_run clears x_pending, the asynchronous entry points do not)
        if (m.host.x_pending) HIP_TRY(hipStreamSynchronize(m.stream));
        std::memcpy(m.host.d_x, host_x, (size_t)m.desc.cols * 4);
        m.host.flush_hdp();  // (sfence, HDP flush register written and read back: the stores are in memory before the launch's doorbell)
        m.host.x_pending = true;
        m.host.d_x_cur = m.host.d_x;
        m.host.have_query = true;
        if (elapsed_ns)
            *elapsed_ns = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::high_resolution_clock::now() - t0).count();
        return TKSPMV_OK;
    }
    if (m.host.host_path && m.host.h_x) {
        // (an earlier upload from the staging copy must have been consumed before it is overwritten)
        if (m.host.x_pending) HIP_TRY(hipStreamSynchronize(m.stream));
        std::memcpy(m.host.h_x, host_x, (size_t)m.desc.cols * 4);
        if (!m.host.host_x_direct) {
            HIP_TRY(hipMemcpyAsync(m.host.d_x, m.host.h_x, (size_t)m.desc.cols * 4, hipMemcpyHostToDevice, m.stream));
            HIP_TRY(hipEventRecord(m.ev2, m.stream));  // a launch on another stream waits for this upload (order_x)
        }
        m.host.x_pending = true;
        m.host.d_x_cur = m.host.host_x_direct ? m.host.h_x_dev : m.host.d_x;
        m.host.have_query = true;
        if (elapsed_ns)
            *elapsed_ns = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::high_resolution_clock::now() - t0).count();
        return TKSPMV_OK;
    } else {
        HIP_TRY(hipMemcpyAsync(m.host.d_x, host_x, (size_t)m.desc.cols * 4, hipMemcpyHostToDevice, m.stream));
        HIP_TRY(hipStreamSynchronize(m.stream));
    }
    m.host.d_x_cur = m.host.d_x;
    m.host.have_query = true;
    if (elapsed_ns)
        *elapsed_ns = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::high_resolution_clock::now() - t0)
                          .count();
    return TKSPMV_OK;
}

int Engine::set_query_device(const float *dev_x, std::string &err) {
    if (!dev_x) return fail(err, TKSPMV_ERR_INVALID, "query vector is NULL");
    impl_->host.d_x_cur = dev_x;
    impl_->host.have_query = true;
    return TKSPMV_OK;
}

// What every enqueue_* entry and drain do around their launches. In front: the stream (the caller's, or the engine's own) and the
// device. Behind: the launches' error and, for the entries that write a result pair, the marks tkspmv_read goes by.
template <class Launch>
static int enqueue_on(EngineImpl &m, void *stream, bool writes_result, std::string &err, Launch launch) {
    hipStream_t s = stream ? (hipStream_t)stream : m.stream;
    HIP_TRY(hipSetDevice(m.device));
    if (const int st = launch(s)) return st;
    HIP_TRY(hipGetLastError());
    if (writes_result) m.host.result_on_device();
    return TKSPMV_OK;
}

int Engine::enqueue(const float *dev_x, uint32_t *dev_idx, float *dev_val, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = m.resolve_query(dev_x, 1, err)) return st;
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        HIP_TRY(m.order_x(dev_x, s));
        m.launch_query(dev_x, dev_idx ? dev_idx : m.host.d_out_idx, dev_val ? dev_val : m.host.d_out_val, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_many(const float *dev_xs, int32_t n_x, int32_t count, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || n_x < 1 || count < 0) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_many");
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        const SequenceLists L(m, dev_xs, n_x, count);
        m.launch_sequence(L.xs.data(), L.oi.data(), L.ov.data(), count, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_batch(const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream,
                          std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || count < 0 || (dev_idx == nullptr) != (dev_val == nullptr)) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_batch");
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        const SequenceLists L(m, dev_xs, count > 0 ? count : 1, count, dev_idx, dev_val);
        m.launch_sequence(L.xs.data(), L.oi.data(), L.ov.data(), count, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_list(const float *const *dev_xs, uint32_t *const *dev_idx, float *const *dev_val, int32_t count,
                         void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || !dev_idx || !dev_val || count < 0) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_list");
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        m.launch_sequence(dev_xs, dev_idx, dev_val, count, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_multi(const float *dev_xs, int32_t count, uint32_t *dev_idx, float *dev_val, void *stream,
                          std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs && count == 1) dev_xs = m.host.d_x_cur;  // the vector installed by tkspmv_set_query / set_query_device
    if (!dev_xs || count < 0 || (dev_idx == nullptr) != (dev_val == nullptr)) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_multi");
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        const SequenceLists L(m, dev_xs, count > 0 ? count : 1, count, dev_idx, dev_val);
        m.launch_multi_sequence(L.xs.data(), L.oi.data(), L.ov.data(), count, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_multi_list(const float *const *dev_xs, uint32_t *const *dev_idx, float *const *dev_val, int32_t count,
                               void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || !dev_idx || !dev_val || count < 0) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_multi_list");
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        m.launch_multi_sequence(dev_xs, dev_idx, dev_val, count, s);
        return TKSPMV_OK;
    });
}

int Engine::set_filter(const uint32_t *host_mask, std::string &err) {
    EngineImpl &m = *impl_;
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(hipStreamSynchronize(m.stream));  // (a filtered query enqueued earlier may still read the installed mask)
    if (!host_mask) {
        m.filter.have_filter = false;
        return TKSPMV_OK;
    }
    if (!m.filter.d_filter) HIP_TRY(m.alloc(m.filter.d_filter, (size_t)m.mask_words() * 4));
    HIP_TRY(hipMemcpy(m.filter.d_filter, host_mask, (size_t)m.mask_words() * 4, hipMemcpyHostToDevice));
    m.filter.have_filter = true;
    return TKSPMV_OK;
}

int Engine::enqueue_filtered(const float *dev_xs, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx,
                             float *dev_val, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (const char *why = m.filter_unsupported()) return fail(err, TKSPMV_ERR_UNSUPPORTED, why);
    if (count < 1 || mask_stride_words < 0 || (dev_idx == nullptr) != (dev_val == nullptr))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_filtered (count >= 1, mask_stride_words >= 0, dev_idx and dev_val both given or both NULL)");
    if (!dev_mask && !m.filter.have_filter) return fail(err, TKSPMV_ERR_INVALID, "no allow-mask given and none installed (tkspmv_set_filter)");
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        if (const int st = m.settle_before_owned_result(true, err)) return st;  // (whatever buffers the call names: unconditionally)
        HIP_TRY(m.order_x(dev_xs, s));
        const SequenceLists L(m, dev_xs, count, count, dev_idx, dev_val);
        m.launch_filtered(L.xs.data(), dev_mask ? dev_mask : m.filter.d_filter, m.stride_of(dev_mask, mask_stride_words), L.oi.data(), L.ov.data(), count, s);
        return TKSPMV_OK;
    });
}

int Engine::set_groups(const uint32_t *host_groups, uint32_t n_groups, std::string &err) {
    EngineImpl &m = *impl_;
    EngineImpl::Grouped &Q = m.grouped;
    if (host_groups) {  // checked before any device call: a bad label installs nothing
        if (n_groups == 0u) return fail(err, TKSPMV_ERR_INVALID, "n_groups must be at least 1");
        for (uint32_t r = 0; r < m.desc.rows; ++r)
            if (host_groups[r] >= n_groups) return fail(err, TKSPMV_ERR_INVALID, "group label of row " + std::to_string(r) + " is " + std::to_string(host_groups[r]) + ": labels must be below n_groups = " + std::to_string(n_groups));
    }
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(hipStreamSynchronize(m.stream));  // (a grouped query enqueued earlier may still read the installed labels)
    if (!host_groups) {
        Q.have_groups = false;
        return TKSPMV_OK;
    }
    Q.have_groups = false;  // (until everything below has succeeded)
    const size_t rows = std::max<size_t>(m.desc.rows, 1);
    if (!Q.d_groups) HIP_TRY(m.alloc(Q.d_groups, rows * 4));
    if (!Q.d_gy) HIP_TRY(m.alloc_ninf_scores(Q.d_gy));
    if (!Q.d_gwords) HIP_TRY(m.alloc(Q.d_gwords, (size_t)EngineImpl::SelectWords::N_WORDS * 4, Mem::Device, 0));
    if (!Q.d_gout_grp) HIP_TRY(m.alloc(Q.d_gout_grp, (size_t)m.desc.k * 4, Mem::Device, 0xFF));
    if (!Q.d_gout_n) HIP_TRY(m.alloc(Q.d_gout_n, 4, Mem::Device, 0));
    if (n_groups > Q.group_cap) {
        HIP_TRY(m.grow_scratch(Q.group_cap, n_groups, {{(void **)&Q.d_gkey, (size_t)n_groups * 8}, {(void **)&Q.d_gscore, (size_t)n_groups * 4},
                                                      {(void **)&Q.d_grow, (size_t)n_groups * 4}, {(void **)&Q.d_gcand, (size_t)n_groups * 8}}));
        HIP_TRY(hipMemset(Q.d_gkey, 0, (size_t)n_groups * 8));
    }
    HIP_TRY(hipMemcpy(Q.d_groups, host_groups, (size_t)m.desc.rows * 4, hipMemcpyHostToDevice));
    Q.n_groups = n_groups;
    Q.have_groups = true;
    return TKSPMV_OK;
}

// The boost of a boosted call: the caller's arrays, or -- both NULL -- the installed pair, one for every query (STATE if none is).
static int resolve_boost(const EngineImpl &m, const float *dev_weight, const float *dev_bias, int64_t boost_stride, EngineImpl::BoostSpec &spec, std::string &err) {
    spec = EngineImpl::BoostSpec{dev_weight, dev_bias, (size_t)boost_stride};
    if (dev_weight || dev_bias) return TKSPMV_OK;
    if (!m.boost.have_weight && !m.boost.have_bias) return fail(err, TKSPMV_ERR_STATE, "no boost installed (call tkspmv_set_boost first, or give dev_weight / dev_bias)");
    spec = EngineImpl::BoostSpec{m.boost.have_weight ? m.boost.d_weight : nullptr, m.boost.have_bias ? m.boost.d_bias : nullptr, 0u};
    return TKSPMV_OK;
}

// Grouped queries, plain or boosted: the argument checks, the error order and the launch are one.
static int enqueue_groups(EngineImpl &m, const char *what, const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                          bool boosted, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp,
                          uint32_t *dev_n, void *stream, std::string &err) {
    if (count < 1 || boost_stride < 0 || mask_stride_words < 0 || (dev_idx == nullptr) != (dev_val == nullptr) || (dev_idx == nullptr) != (dev_grp == nullptr))
        return fail(err, TKSPMV_ERR_INVALID, std::string("bad arguments to ") + what + " (count >= 1, strides >= 0, dev_idx, dev_val and dev_grp all given or all NULL)");
    if (boosted && !dev_xs && count != 1) return fail(err, TKSPMV_ERR_INVALID, "dev_xs = NULL takes the installed query vector: count must be 1");
    if (const char *why = m.grouped_unsupported(dev_mask != nullptr)) return fail(err, TKSPMV_ERR_UNSUPPORTED, why);
    EngineImpl::BoostSpec spec{};
    if (boosted)
        if (const int st = resolve_boost(m, dev_weight, dev_bias, boost_stride, spec, err)) return st;
    if (!m.grouped.have_groups) return fail(err, TKSPMV_ERR_STATE, "no group labels installed (call tkspmv_set_groups first)");
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    const bool own = dev_idx == nullptr;  // the engine-owned result pair, group ids and n: the last query wins
    return enqueue_on(m, stream, own, err, [&](hipStream_t s) -> int {
        if (const int st = m.settle_before_owned_result(own, err)) return st;
        HIP_TRY(m.order_x(dev_xs, s));
        const size_t k = own ? 0u : (size_t)m.desc.k;
        m.launch_grouped(dev_xs, count, dev_mask, m.stride_of(dev_mask, mask_stride_words), own ? m.host.d_out_idx : dev_idx, own ? m.host.d_out_val : dev_val,
                         own ? m.grouped.d_gout_grp : dev_grp, k, dev_n ? dev_n : m.grouped.d_gout_n, dev_n ? 1u : 0u, s, boosted ? &spec : nullptr);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_grouped(const float *dev_xs, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx,
                            float *dev_val, uint32_t *dev_grp, uint32_t *dev_n, void *stream, std::string &err) {
    return enqueue_groups(*impl_, "enqueue_grouped", dev_xs, count, nullptr, nullptr, 0, false, dev_mask, mask_stride_words, dev_idx, dev_val, dev_grp, dev_n, stream, err);
}

int Engine::enqueue_boosted_grouped(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                    const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val, uint32_t *dev_grp, uint32_t *dev_n,
                                    void *stream, std::string &err) {
    return enqueue_groups(*impl_, "enqueue_boosted_grouped", dev_xs, count, dev_weight, dev_bias, boost_stride, true, dev_mask, mask_stride_words, dev_idx, dev_val,
                          dev_grp, dev_n, stream, err);
}

// The host forms of the two: the installed vector, mask and labels (and boost); waits.
static int run_groups(EngineImpl &m, bool boosted, int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n, std::string &err) {
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err)) return st;
    if (const int st = enqueue_groups(m, boosted ? "run_boosted_grouped" : "run_grouped", nullptr, 1, nullptr, nullptr, 0, boosted, mask, 0, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, err))
        return st;
    if (const int st = m.finish_host_form(err)) return st;
    const size_t k = (size_t)m.desc.k;
    uint32_t found = 0u;
    HIP_TRY(hipMemcpy(&found, m.grouped.d_gout_n, 4, hipMemcpyDeviceToHost));
    if (idx) HIP_TRY(hipMemcpy(idx, m.host.d_out_idx, k * 4, hipMemcpyDeviceToHost));
    if (val) HIP_TRY(hipMemcpy(val, m.host.d_out_val, k * 4, hipMemcpyDeviceToHost));
    if (grp) HIP_TRY(hipMemcpy(grp, m.grouped.d_gout_grp, k * 4, hipMemcpyDeviceToHost));
    if (n) *n = (int32_t)found;
    return TKSPMV_OK;
}

int Engine::run_grouped(int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n, std::string &err) {
    return run_groups(*impl_, false, use_filter, idx, val, grp, n, err);
}

int Engine::run_boosted_grouped(int32_t use_filter, uint32_t *idx, float *val, uint32_t *grp, int32_t *n, std::string &err) {
    return run_groups(*impl_, true, use_filter, idx, val, grp, n, err);
}

// Search-after pages, plain (boost NULL, both arrays NULL) or boosted: the argument checks, the error order and the launch are one.
static int enqueue_pages(EngineImpl &m, const char *what, const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                         bool boosted, const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx,
                         float *dev_val, uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream, std::string &err) {
    if (count < 1 || boost_stride < 0 || mask_stride_words < 0 || (dev_idx == nullptr) != (dev_val == nullptr))
        return fail(err, TKSPMV_ERR_INVALID, std::string("bad arguments to ") + what + " (count >= 1, strides >= 0, dev_idx and dev_val both given or both NULL)");
    if (!dev_xs && count != 1) return fail(err, TKSPMV_ERR_INVALID, "dev_xs = NULL takes the installed query vector: count must be 1");
    if (const char *why = m.grouped_unsupported(dev_mask != nullptr)) return fail(err, TKSPMV_ERR_UNSUPPORTED, std::string("search-after queries take the grouped queries' route: ") + why);
    EngineImpl::BoostSpec spec{};
    if (boosted)
        if (const int st = resolve_boost(m, dev_weight, dev_bias, boost_stride, spec, err)) return st;
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    const bool own = dev_idx == nullptr;  // the engine-owned result pair: the last query wins
    return enqueue_on(m, stream, own, err, [&](hipStream_t s) -> int {
        if (const int st = m.settle_before_owned_result(own, err)) return st;
        HIP_TRY(m.ensure_after());
        HIP_TRY(m.order_x(dev_xs, s));
        m.launch_after(dev_xs, count, dev_cursors, dev_mask, m.stride_of(dev_mask, mask_stride_words), own ? m.host.d_out_idx : dev_idx,
                       own ? m.host.d_out_val : dev_val, own ? 0u : (size_t)m.desc.k, dev_n, dev_total, dev_next, s, boosted ? &spec : nullptr);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_after(const float *dev_xs, int32_t count, const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words,
                          uint32_t *dev_idx, float *dev_val, uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream, std::string &err) {
    return enqueue_pages(*impl_, "enqueue_after", dev_xs, count, nullptr, nullptr, 0, false, dev_cursors, dev_mask, mask_stride_words, dev_idx, dev_val, dev_n,
                         dev_total, dev_next, stream, err);
}

int Engine::enqueue_boosted(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                            const tkspmv_cursor *dev_cursors, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                            uint32_t *dev_n, uint32_t *dev_total, tkspmv_cursor *dev_next, void *stream, std::string &err) {
    return enqueue_pages(*impl_, "enqueue_boosted", dev_xs, count, dev_weight, dev_bias, boost_stride, true, dev_cursors, dev_mask, mask_stride_words, dev_idx,
                         dev_val, dev_n, dev_total, dev_next, stream, err);
}

// The host forms of the two: the installed vector, a host cursor, the installed mask (and boost); waits.
static int run_page(EngineImpl &m, bool boosted, const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total,
                    tkspmv_cursor *next, std::string &err) {
    using After = EngineImpl::After;
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err)) return st;
    if (const char *why = m.grouped_unsupported(use_filter != 0)) return fail(err, TKSPMV_ERR_UNSUPPORTED, std::string("search-after queries take the grouped queries' route: ") + why);
    if (!m.host.d_x_cur) return fail(err, TKSPMV_ERR_STATE, "no query vector installed (call tkspmv_set_query first)");
    if (boosted && !m.boost.have_weight && !m.boost.have_bias) return fail(err, TKSPMV_ERR_STATE, "no boost installed (call tkspmv_set_boost first)");
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(m.ensure_after());
    uint32_t *const out = m.after.d_aout;
    // (the cursor words belong to these host forms alone, and the host form before this one has waited)
    if (cursor) HIP_TRY(hipMemcpy(out + After::O_CURSOR, cursor, sizeof(tkspmv_cursor), hipMemcpyHostToDevice));
    if (const int st = enqueue_pages(m, boosted ? "run_boosted" : "run_after", nullptr, 1, nullptr, nullptr, 0, boosted,
                                     cursor ? reinterpret_cast<const tkspmv_cursor *>(out + After::O_CURSOR) : nullptr, mask, 0, nullptr, nullptr,
                                     out + After::O_N, out + After::O_TOTAL, reinterpret_cast<tkspmv_cursor *>(out + After::O_NEXT), nullptr, err))
        return st;
    if (const int st = m.finish_host_form(err)) return st;
    const size_t k = (size_t)m.desc.k;
    uint32_t words[After::N_OUT];
    HIP_TRY(hipMemcpy(words, out, sizeof(words), hipMemcpyDeviceToHost));
    if (idx) HIP_TRY(hipMemcpy(idx, m.host.d_out_idx, k * 4, hipMemcpyDeviceToHost));
    if (val) HIP_TRY(hipMemcpy(val, m.host.d_out_val, k * 4, hipMemcpyDeviceToHost));
    if (n) *n = (int32_t)words[After::O_N];
    if (total) *total = words[After::O_TOTAL];
    if (next) std::memcpy(next, words + After::O_NEXT, sizeof(tkspmv_cursor));
    return TKSPMV_OK;
}

int Engine::run_after(const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total, tkspmv_cursor *next,
                      std::string &err) {
    return run_page(*impl_, false, cursor, use_filter, idx, val, n, total, next, err);
}

int Engine::run_boosted(const tkspmv_cursor *cursor, int32_t use_filter, uint32_t *idx, float *val, int32_t *n, uint32_t *total, tkspmv_cursor *next,
                        std::string &err) {
    return run_page(*impl_, true, cursor, use_filter, idx, val, n, total, next, err);
}

int Engine::set_boost(const float *host_weight, const float *host_bias, std::string &err) {
    EngineImpl &m = *impl_;
    EngineImpl::Boost &Q = m.boost;
    for (const float *a : {host_weight, host_bias})  // checked before any device call: a bad entry installs nothing
        for (uint32_t r = 0; a && r < m.desc.rows; ++r)
            if (!std::isfinite(a[r]))
                return fail(err, TKSPMV_ERR_INVALID, std::string(a == host_weight ? "weight" : "bias") + " of row " + std::to_string(r) + " is not finite");
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(hipStreamSynchronize(m.stream));  // (a boosted query enqueued earlier may still read the installed arrays)
    Q.have_weight = Q.have_bias = false;  // (until everything below has succeeded; both NULL: removed)
    const size_t bytes = std::max<size_t>(m.desc.rows, 1) * 4;
    if (host_weight && !Q.d_weight) HIP_TRY(m.alloc(Q.d_weight, bytes));
    if (host_bias && !Q.d_bias) HIP_TRY(m.alloc(Q.d_bias, bytes));
    if (host_weight) HIP_TRY(hipMemcpy(Q.d_weight, host_weight, (size_t)m.desc.rows * 4, hipMemcpyHostToDevice));
    if (host_bias) HIP_TRY(hipMemcpy(Q.d_bias, host_bias, (size_t)m.desc.rows * 4, hipMemcpyHostToDevice));
    Q.have_weight = host_weight != nullptr;
    Q.have_bias = host_bias != nullptr;
    return TKSPMV_OK;
}

int Engine::enqueue_range(const float *dev_xs, int32_t count, const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words,
                          uint32_t *dev_idx, float *dev_val, uint32_t capacity, uint32_t *dev_counts, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (m.range_unsupported(err)) return TKSPMV_ERR_UNSUPPORTED;
    if (count < 1 || !dev_thresholds || !dev_counts || mask_stride_words < 0 || (dev_idx == nullptr) != (dev_val == nullptr) ||
        (capacity > 0u && !dev_idx) || (capacity == 0u && dev_idx))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_range (count >= 1, thresholds and counts given, mask_stride_words >= 0, dev_idx and "
                                             "dev_val both given with capacity > 0 or both NULL with capacity = 0)");
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written: tkspmv_read's view stays)
        HIP_TRY(m.order_x(dev_xs, s));
        m.launch_range(dev_xs, count, dev_thresholds, dev_mask, m.stride_of(dev_mask, mask_stride_words), dev_idx, dev_val, capacity, dev_counts, s);
        return TKSPMV_OK;
    });
}

// A boosted threshold form's own checks, in tkspmv_enqueue_boosted's order: UNSUPPORTED by the grouped queries' rule, then STATE for
// a missing boost.
static int boosted_form_scope(const EngineImpl &m, bool with_mask, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                              EngineImpl::BoostSpec &spec, std::string &err) {
    if (const char *why = m.grouped_unsupported(with_mask)) return fail(err, TKSPMV_ERR_UNSUPPORTED, std::string("boosted thresholds take the grouped queries' route: ") + why);
    return resolve_boost(m, dev_weight, dev_bias, boost_stride, spec, err);
}

int Engine::enqueue_boosted_range(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                  const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words, uint32_t *dev_idx, float *dev_val,
                                  uint32_t capacity, uint32_t *dev_counts, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (count < 1 || boost_stride < 0 || !dev_thresholds || !dev_counts || mask_stride_words < 0 || (dev_idx == nullptr) != (dev_val == nullptr) ||
        (capacity > 0u && !dev_idx) || (capacity == 0u && dev_idx))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_boosted_range (count >= 1, thresholds and counts given, strides >= 0, dev_idx and "
                                             "dev_val both given with capacity > 0 or both NULL with capacity = 0)");
    if (!dev_xs && count != 1) return fail(err, TKSPMV_ERR_INVALID, "dev_xs = NULL takes the installed query vector: count must be 1");
    EngineImpl::BoostSpec spec{};
    if (const int st = boosted_form_scope(m, dev_mask != nullptr, dev_weight, dev_bias, boost_stride, spec, err)) return st;
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written: tkspmv_read's view stays)
        HIP_TRY(m.ensure_after());
        HIP_TRY(m.order_x(dev_xs, s));
        m.launch_boosted_range(dev_xs, count, dev_thresholds, spec, dev_mask, m.stride_of(dev_mask, mask_stride_words), dev_idx, dev_val, capacity, dev_counts, s);
        return TKSPMV_OK;
    });
}

// The host forms of the two range calls: the installed vector (and boost), a host threshold, the installed mask; waits and sorts.
static int run_range_form(Engine &e, EngineImpl &m, bool boosted, float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count,
                          std::string &err) {
    if (!boosted && m.range_unsupported(err)) return TKSPMV_ERR_UNSUPPORTED;
    if (!count || (idx == nullptr) != (val == nullptr) || (capacity > 0u && !idx) || (capacity == 0u && idx))
        return fail(err, TKSPMV_ERR_INVALID, std::string("bad arguments to ") + (boosted ? "run_boosted_range" : "run_range") +
                                                 " (count given, idx and val both given with capacity > 0 or both NULL with capacity = 0)");
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err)) return st;
    EngineImpl::BoostSpec spec{};
    if (boosted)
        if (const int st = boosted_form_scope(m, use_filter != 0, nullptr, nullptr, 0, spec, err)) return st;
    const float *installed = nullptr;
    if (const int st = m.resolve_query(installed, 1, err)) return st;
    HIP_TRY(hipSetDevice(m.device));
    if (!m.range.d_range_word) HIP_TRY(m.alloc(m.range.d_range_word, 128, Mem::Device, 0));
    if (capacity > m.range.range_cap) {
        HIP_TRY(hipStreamSynchronize(m.stream));  // (an earlier call's launch is long complete: run_range waits itself)
        HIP_TRY(m.grow_scratch(m.range.range_cap, capacity, {{(void **)&m.range.d_range_idx, (size_t)capacity * 4}, {(void **)&m.range.d_range_val, (size_t)capacity * 4}}));
    }
    HIP_TRY(hipMemcpy(m.range.d_range_word, &threshold, 4, hipMemcpyHostToDevice));
    const float *const tau = reinterpret_cast<const float *>(m.range.d_range_word);
    uint32_t *const d_idx = capacity ? m.range.d_range_idx : nullptr;
    float *const d_val = capacity ? m.range.d_range_val : nullptr;
    if (const int st = boosted ? e.enqueue_boosted_range(nullptr, 1, nullptr, nullptr, 0, tau, mask, 0, d_idx, d_val, capacity, m.range.d_range_word + 1, nullptr, err)
                               : e.enqueue_range(nullptr, 1, tau, mask, 0, d_idx, d_val, capacity, m.range.d_range_word + 1, nullptr, err))
        return st;
    if (const int st = m.finish_host_form(err)) return st;
    uint32_t found = 0u;
    HIP_TRY(hipMemcpy(&found, m.range.d_range_word + 1, 4, hipMemcpyDeviceToHost));
    *count = found;
    const size_t kept = std::min<size_t>(found, capacity);
    if (kept) {
        HIP_TRY(hipMemcpy(idx, m.range.d_range_idx, kept * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(val, m.range.d_range_val, kept * 4, hipMemcpyDeviceToHost));
        sort_tuples(kept, idx, val);
    }
    return TKSPMV_OK;
}

int Engine::run_range(float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count, std::string &err) {
    return run_range_form(*this, *impl_, false, threshold, use_filter, idx, val, capacity, count, err);
}

int Engine::run_boosted_range(float threshold, int32_t use_filter, uint32_t *idx, float *val, uint32_t capacity, uint64_t *count, std::string &err) {
    return run_range_form(*this, *impl_, true, threshold, use_filter, idx, val, capacity, count, err);
}

int Engine::enqueue_facets(const float *dev_xs, int32_t count, const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words,
                           const uint32_t *dev_labels, uint32_t n_bins, uint32_t *dev_counts, tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream,
                           std::string &err) {
    EngineImpl &m = *impl_;
    if (count < 1 || !dev_thresholds || !dev_counts || mask_stride_words < 0 || (dev_labels != nullptr) != (n_bins != 0u) || n_bins > (1u << 30) ||
        (reinterpret_cast<uintptr_t>(dev_best) & 7u) != 0u)
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_facets (count >= 1, thresholds and counts given, mask_stride_words >= 0, dev_labels with "
                                             "1 <= n_bins <= 2^30 or dev_labels = NULL with n_bins = 0, dev_best 8-byte aligned)");
    if (!dev_xs && count != 1) return fail(err, TKSPMV_ERR_INVALID, "dev_xs = NULL takes the installed query vector: count must be 1");
    if (m.range_unsupported(err)) return TKSPMV_ERR_UNSUPPORTED;
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    if (!dev_labels) {
        if (!m.grouped.have_groups) return fail(err, TKSPMV_ERR_STATE, "no labels given and none installed (call tkspmv_set_groups first)");
        dev_labels = m.grouped.d_groups;
        n_bins = m.grouped.n_groups;
    }
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written: tkspmv_read's view stays)
        HIP_TRY(m.order_x(dev_xs, s));
        m.launch_facets(dev_xs, count, dev_thresholds, dev_mask, m.stride_of(dev_mask, mask_stride_words), dev_labels, n_bins, dev_counts, dev_best, dev_totals, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_boosted_facets(const float *dev_xs, int32_t count, const float *dev_weight, const float *dev_bias, int64_t boost_stride,
                                   const float *dev_thresholds, const uint32_t *dev_mask, int64_t mask_stride_words, const uint32_t *dev_labels, uint32_t n_bins,
                                   uint32_t *dev_counts, tkspmv_facet_best *dev_best, uint32_t *dev_totals, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (count < 1 || boost_stride < 0 || !dev_thresholds || !dev_counts || mask_stride_words < 0 || (dev_labels != nullptr) != (n_bins != 0u) || n_bins > (1u << 30) ||
        (reinterpret_cast<uintptr_t>(dev_best) & 7u) != 0u)
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_boosted_facets (count >= 1, thresholds and counts given, strides >= 0, dev_labels with "
                                             "1 <= n_bins <= 2^30 or dev_labels = NULL with n_bins = 0, dev_best 8-byte aligned)");
    if (!dev_xs && count != 1) return fail(err, TKSPMV_ERR_INVALID, "dev_xs = NULL takes the installed query vector: count must be 1");
    EngineImpl::BoostSpec spec{};
    if (const int st = boosted_form_scope(m, dev_mask != nullptr, dev_weight, dev_bias, boost_stride, spec, err)) return st;
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    if (!dev_labels) {
        if (!m.grouped.have_groups) return fail(err, TKSPMV_ERR_STATE, "no labels given and none installed (call tkspmv_set_groups first)");
        dev_labels = m.grouped.d_groups;
        n_bins = m.grouped.n_groups;
    }
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written: tkspmv_read's view stays)
        HIP_TRY(m.ensure_after());
        HIP_TRY(m.order_x(dev_xs, s));
        m.launch_boosted_facets(dev_xs, count, dev_thresholds, spec, dev_mask, m.stride_of(dev_mask, mask_stride_words), dev_labels, n_bins, dev_counts, dev_best,
                                dev_totals, s);
        return TKSPMV_OK;
    });
}

// The host forms of the two facet calls: the installed vector and labels (and boost), a host threshold, the installed mask; waits.
static int run_facets_form(Engine &e, EngineImpl &m, bool boosted, float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total,
                           std::string &err) {
    if (!boosted && m.range_unsupported(err)) return TKSPMV_ERR_UNSUPPORTED;
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err)) return st;
    EngineImpl::BoostSpec spec{};
    if (boosted)
        if (const int st = boosted_form_scope(m, use_filter != 0, nullptr, nullptr, 0, spec, err)) return st;
    const float *installed = nullptr;
    if (const int st = m.resolve_query(installed, 1, err)) return st;
    if (!m.grouped.have_groups) return fail(err, TKSPMV_ERR_STATE, "no labels installed (call tkspmv_set_groups first)");
    HIP_TRY(hipSetDevice(m.device));
    const uint32_t n_bins = m.grouped.n_groups;
    if (!m.range.d_range_word) HIP_TRY(m.alloc(m.range.d_range_word, 128, Mem::Device, 0));
    if (n_bins > m.range.facet_cap) {
        HIP_TRY(hipStreamSynchronize(m.stream));  // (an earlier call's launch is long complete: run_facets waits itself)
        HIP_TRY(m.grow_scratch(m.range.facet_cap, n_bins, {{(void **)&m.range.d_facet_counts, (size_t)n_bins * 4}, {(void **)&m.range.d_facet_best, (size_t)n_bins * 8}}));
    }
    HIP_TRY(hipMemcpy(m.range.d_range_word + 2, &threshold, 4, hipMemcpyHostToDevice));
    const float *const tau = reinterpret_cast<const float *>(m.range.d_range_word + 2);
    tkspmv_facet_best *const d_best = best ? m.range.d_facet_best : nullptr;
    if (const int st = boosted ? e.enqueue_boosted_facets(nullptr, 1, nullptr, nullptr, 0, tau, mask, 0, nullptr, 0u, m.range.d_facet_counts, d_best,
                                                          m.range.d_range_word + 3, nullptr, err)
                               : e.enqueue_facets(nullptr, 1, tau, mask, 0, nullptr, 0u, m.range.d_facet_counts, d_best, m.range.d_range_word + 3, nullptr, err))
        return st;
    if (const int st = m.finish_host_form(err)) return st;
    uint32_t found = 0u;
    HIP_TRY(hipMemcpy(&found, m.range.d_range_word + 3, 4, hipMemcpyDeviceToHost));
    if (total) *total = found;
    if (counts) HIP_TRY(hipMemcpy(counts, m.range.d_facet_counts, (size_t)n_bins * 4, hipMemcpyDeviceToHost));
    if (best) HIP_TRY(hipMemcpy(best, m.range.d_facet_best, (size_t)n_bins * 8, hipMemcpyDeviceToHost));
    return TKSPMV_OK;
}

int Engine::run_facets(float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total, std::string &err) {
    return run_facets_form(*this, *impl_, false, threshold, use_filter, counts, best, total, err);
}

int Engine::run_boosted_facets(float threshold, int32_t use_filter, uint32_t *counts, tkspmv_facet_best *best, uint64_t *total, std::string &err) {
    return run_facets_form(*this, *impl_, true, threshold, use_filter, counts, best, total, err);
}

int Engine::enqueue_match(const uint32_t *dev_clauses, int64_t clause_stride_words, const tkspmv_match *dev_preds, int32_t count, const uint32_t *dev_mask,
                          int64_t mask_stride_words, uint32_t *dev_out, int64_t out_stride_words, uint32_t *dev_counts, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    const int64_t words = (int64_t)m.mask_words();
    if (!dev_clauses || !dev_preds || !dev_out || count < 1 || clause_stride_words < 0 || mask_stride_words < 0 || out_stride_words < 0 ||
        (clause_stride_words != 0 && clause_stride_words < (int64_t)m.desc.cols) || (out_stride_words < words && !(out_stride_words == 0 && count == 1)))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_match (table, predicates and output given, count >= 1, strides >= 0, clause_stride_words 0 or "
                                             ">= cols, out_stride_words >= ceil(rows / 32) or 0 with count = 1)");
    if (const char *why = m.match_unsupported(dev_mask != nullptr)) return fail(err, TKSPMV_ERR_UNSUPPORTED, why);
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written: tkspmv_read's view stays)
        m.launch_match(dev_clauses, (size_t)clause_stride_words, dev_preds, count, dev_mask, m.stride_of(dev_mask, mask_stride_words), dev_out,
                       (size_t)out_stride_words, dev_counts, s);
        return TKSPMV_OK;
    });
}

int Engine::run_match(const uint32_t *host_clauses, const tkspmv_match *pred, int32_t use_filter, int32_t install, uint32_t *host_mask, uint64_t *count,
                      std::string &err) {
    EngineImpl &m = *impl_;
    if (!host_clauses || !pred) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to run_match (clause table and predicate given)");
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err)) return st;
    if (const char *why = m.match_unsupported(use_filter != 0)) return fail(err, TKSPMV_ERR_UNSUPPORTED, why);
    HIP_TRY(hipSetDevice(m.device));
    const size_t cols = m.desc.cols, words = m.mask_words();
    if (!m.match.d_match_in) HIP_TRY(m.alloc(m.match.d_match_in, (cols + 5u) * 4, Mem::Device, 0));
    if (!m.match.d_match_out) HIP_TRY(m.alloc(m.match.d_match_out, words * 4, Mem::Device, 0));
    // (the scratch belongs to this host form alone, and the host form before this one has waited)
    HIP_TRY(hipMemcpy(m.match.d_match_in, host_clauses, cols * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m.match.d_match_in + cols, pred, sizeof(tkspmv_match), hipMemcpyHostToDevice));
    if (const int st = enqueue_match(m.match.d_match_in, 0, reinterpret_cast<const tkspmv_match *>(m.match.d_match_in + cols), 1, mask, 0, m.match.d_match_out, 0,
                                     m.match.d_match_in + cols + 4, nullptr, err))
        return st;
    // (no query vector was read: x_pending stays -- clearing it could free the staging copy under a query in flight on a caller's stream)
    if (const int st = m.wait_idle(err)) return st;
    uint32_t found = 0u;
    HIP_TRY(hipMemcpy(&found, m.match.d_match_in + cols + 4, 4, hipMemcpyDeviceToHost));
    if (count) *count = found;
    if (host_mask) HIP_TRY(hipMemcpy(host_mask, m.match.d_match_out, words * 4, hipMemcpyDeviceToHost));
    if (install) {  // (as tkspmv_set_filter installs a mask; nothing enqueued on the engine's stream still reads the old one: it has just idled)
        if (!m.filter.d_filter) HIP_TRY(m.alloc(m.filter.d_filter, words * 4));
        HIP_TRY(hipMemcpy(m.filter.d_filter, m.match.d_match_out, words * 4, hipMemcpyDeviceToDevice));
        m.filter.have_filter = true;
    }
    return TKSPMV_OK;
}

// What both entries of a whole-matrix operation -- tkspmv_enqueue_X on device pointers, tkspmv_X on host pointers -- test first, one
// function per operation: the arguments (INVALID; the message carries the entry's name), then the stored rows' scope (UNSUPPORTED).
// (Label sums and column statistics keep two argument checks each: the enqueue forms test alignment and flags, sets and strides,
// which the host forms do not have, and each message lists its own rules.)
static int bad_arguments(std::string &err, const char *entry, const std::string &rules) {
    return fail(err, TKSPMV_ERR_INVALID, std::string("bad arguments to ") + entry + " (" + rules + ")");
}
static int check_row_vectors(const EngineImpl &m, const char *entry, const void *rows, const void *xs, int32_t count, std::string &err) {
    return rows && xs && count >= 1 ? m.row_scope(err) : bad_arguments(err, entry, "row ids and vectors given, count >= 1");
}
// (xs_name: "dev_xs" / "host_xs", as the entry's prototype calls the vectors)
static int check_score_rows(const EngineImpl &m, const char *entry, const char *xs_name, const void *xs, int32_t count, const void *rows, int32_t n_rows,
                            int64_t rows_stride, const void *scores, std::string &err) {
    if (!rows || !scores || count < 1 || n_rows < 1 || rows_stride < 0 || (rows_stride != 0 && rows_stride < n_rows))
        return bad_arguments(err, entry, "row ids and scores given, count >= 1, n_rows >= 1, rows_stride = 0 or >= n_rows");
    if (!xs && count != 1) return fail(err, TKSPMV_ERR_INVALID, std::string(xs_name) + " = NULL takes the installed query vector: count must be 1");
    return m.row_scope(err);
}
static int check_row_stats(const EngineImpl &m, const char *entry, const void *out, int32_t kind, std::string &err) {
    if (!out || kind < TKSPMV_ROW_NNZ || kind > TKSPMV_ROW_INV_L2) return bad_arguments(err, entry, "output given, kind = TKSPMV_ROW_NNZ .. TKSPMV_ROW_INV_L2");
    return m.row_scope(err, EngineImpl::STATS_SCOPE);
}
static int check_assign(const EngineImpl &m, const char *entry, const void *xs, const void *labels, int32_t count, std::string &err) {
    return xs && labels && count >= 1 ? m.row_scope(err, EngineImpl::ASSIGN_SCOPE) : bad_arguments(err, entry, "vectors and labels given, count >= 1");
}
// (the one real difference of a pair: tkspmv_enqueue_nearest needs the scores -- later passes merge with them --, tkspmv_nearest keeps
//  them in its scratch and takes host_scores = NULL. with_mask: the call names a mask, whose scope is the filtered queries'.)
static int check_nearest(const EngineImpl &m, const char *entry, const void *xs, const void *labels, const void *scores, bool scores_optional, int32_t count,
                         int32_t n, bool with_mask, std::string &err) {
    if (!xs || !labels || !(scores || scores_optional) || count < 1 || n < 1 || n > TKSPMV_NEAREST_MAX_N)
        return bad_arguments(err, entry, std::string(scores_optional ? "vectors and labels" : "vectors, labels and scores") + " given, count >= 1, n = 1 .. TKSPMV_NEAREST_MAX_N");
    if (const int st = m.row_scope(err, EngineImpl::ASSIGN_SCOPE)) return st;
    const char *why = m.col_stats_unsupported(with_mask);
    return why ? fail(err, TKSPMV_ERR_UNSUPPORTED, std::string("assignment under an allow-mask: ") + why) : TKSPMV_OK;
}

int Engine::enqueue_row_vectors(const uint32_t *dev_rows, int32_t count, float *dev_xs, uint32_t *dev_len, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_row_vectors(m, "enqueue_row_vectors", dev_rows, dev_xs, count, err)) return st;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_row_vectors(dev_rows, count, dev_xs, dev_len, s);
        return TKSPMV_OK;
    });
}

int Engine::row_vectors(const uint32_t *host_rows, int32_t count, float *host_xs, uint32_t *host_len, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_row_vectors(m, "row_vectors", host_rows, host_xs, count, err)) return st;
    HIP_TRY(hipSetDevice(m.device));
    // (buffers of this call alone: the caller asks for `count` whole vectors at once, whatever their size)
    ScratchBuffer<uint32_t> d_rows, d_len;
    ScratchBuffer<float> d_xs;
    const size_t xs_bytes = (size_t)count * m.desc.cols * 4;
    HIP_TRY(hipMalloc((void **)&d_rows.p, (size_t)count * 4));
    HIP_TRY(hipMalloc((void **)&d_len.p, (size_t)count * 4));
    HIP_TRY(hipMalloc((void **)&d_xs.p, xs_bytes));
    HIP_TRY(hipMemcpy(d_rows.p, host_rows, (size_t)count * 4, hipMemcpyHostToDevice));
    m.launch_row_vectors(d_rows.p, count, d_xs.p, d_len.p, m.stream);
    HIP_TRY(hipGetLastError());
    if (const int st = m.wait_idle(err)) return st;  // (the host has just waited for the engine's stream)
    HIP_TRY(hipMemcpy(host_xs, d_xs.p, xs_bytes, hipMemcpyDeviceToHost));
    if (host_len) HIP_TRY(hipMemcpy(host_len, d_len.p, (size_t)count * 4, hipMemcpyDeviceToHost));
    return TKSPMV_OK;
}

int Engine::run_similar(const uint32_t *host_rows, int32_t count, int32_t exclude_self, uint32_t *idx, float *val, std::string &err) {
    EngineImpl &m = *impl_;
    if (!host_rows || !idx || !val || count < 1) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to run_similar (row ids and [count][k] outputs given, count >= 1)");
    if (const int st = m.row_scope(err)) return st;
    HIP_TRY(hipSetDevice(m.device));
    const size_t k = (size_t)m.desc.k, cols = m.desc.cols;
    const uint32_t chunk_max = (uint32_t)std::max<size_t>(1, std::min<size_t>(EngineImpl::Similar::SIMILAR_MAX_ROWS, EngineImpl::Similar::SIMILAR_MAX_BYTES / (cols * 4)));
    const uint32_t want = std::min<uint32_t>((uint32_t)count, chunk_max);
    if (want > m.similar.sim_cap) {
        if (const int st = m.wait_idle(err)) return st;  // (an earlier call's chunks are long complete: run_similar waits itself)
        HIP_TRY(m.grow_scratch(m.similar.sim_cap, want, {{(void **)&m.similar.d_sim_rows, (size_t)want * 4}, {(void **)&m.similar.d_sim_xs, (size_t)want * cols * 4},
                                                 {(void **)&m.similar.d_sim_idx, (size_t)want * k * 4}, {(void **)&m.similar.d_sim_val, (size_t)want * k * 4}}));
    }
    for (int32_t i0 = 0; i0 < count; i0 += (int32_t)m.similar.sim_cap) {
        const int32_t c = std::min<int32_t>((int32_t)m.similar.sim_cap, count - i0);
        // upload ids, row vectors, the batch sequence, then WAIT: under REPAIR=host a trusted batch launch may be repaired from the
        // host's next wait (settle()); the repair reads the query vectors again and writes the results again, so the scratch vectors
        // must not be overwritten and the results not be read before the engine has settled.
        HIP_TRY(hipMemcpy(m.similar.d_sim_rows, host_rows + i0, (size_t)c * 4, hipMemcpyHostToDevice));
        m.launch_row_vectors(m.similar.d_sim_rows, c, m.similar.d_sim_xs, nullptr, m.stream);
        HIP_TRY(hipGetLastError());
        int st = enqueue_batch(m.similar.d_sim_xs, c, m.similar.d_sim_idx, m.similar.d_sim_val, nullptr, err);
        if (st == TKSPMV_OK) st = synchronize(err);
        if (st != TKSPMV_OK) return st;
        HIP_TRY(hipMemcpy(idx + (size_t)i0 * k, m.similar.d_sim_idx, (size_t)c * k * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(val + (size_t)i0 * k, m.similar.d_sim_val, (size_t)c * k * 4, hipMemcpyDeviceToHost));
    }
    if (exclude_self) {
        // the query's own row leaves its list: the rest moves up, the last slot becomes the pad (0, 0.0f)
        for (int32_t i = 0; i < count; ++i) {
            uint32_t *li = idx + (size_t)i * k;
            float *lv = val + (size_t)i * k;
            const uint32_t *hit = std::find(li, li + k, host_rows[i]);
            if (hit == li + k) continue;
            const size_t j = (size_t)(hit - li);
            std::copy(li + j + 1, li + k, li + j);
            std::copy(lv + j + 1, lv + k, lv + j);
            li[k - 1] = 0u;
            lv[k - 1] = 0.0f;
        }
    }
    return TKSPMV_OK;
}

int Engine::enqueue_score_rows(const float *dev_xs, int32_t count, const uint32_t *dev_rows, int32_t n_rows, int64_t rows_stride, float *dev_scores,
                               void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_score_rows(m, "enqueue_score_rows", "dev_xs", dev_xs, count, dev_rows, n_rows, rows_stride, dev_scores, err)) return st;
    if (const int st = m.resolve_query(dev_xs, count, err)) return st;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        HIP_TRY(m.order_x(dev_xs, s));
        m.launch_score_rows(dev_xs, count, dev_rows, n_rows, (size_t)rows_stride, dev_scores, s);
        return TKSPMV_OK;
    });
}

int Engine::score_rows(const float *host_xs, int32_t count, const uint32_t *host_rows, int32_t n_rows, int64_t rows_stride, float *host_scores,
                       std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_score_rows(m, "score_rows", "host_xs", host_xs, count, host_rows, n_rows, rows_stride, host_scores, err)) return st;
    const float *installed = nullptr;
    if (!host_xs) {
        if (const int st = m.resolve_query(installed, 1, err)) return st;
    }
    HIP_TRY(hipSetDevice(m.device));
    typedef EngineImpl::ScoreRows SR;
    const size_t cols = m.desc.cols;
    const uint32_t q_max = (uint32_t)std::max<size_t>(1, std::min<size_t>(SR::SCORE_MAX_QUERIES, SR::SCORE_MAX_BYTES / (cols * 4)));
    const uint32_t want_q = std::min<uint32_t>((uint32_t)count, q_max), want_r = std::min<uint32_t>((uint32_t)n_rows, SR::SCORE_MAX_ROWS);
    if (want_q > m.score.sr_q_cap || want_r > m.score.sr_row_cap) {
        HIP_TRY(hipStreamSynchronize(m.stream));  // (an earlier call's chunks are long complete: score_rows waits itself)
        const uint32_t q_cap = std::max(want_q, m.score.sr_q_cap), r_cap = std::max(want_r, m.score.sr_row_cap);
        uint32_t grown = 0;
        m.score.sr_q_cap = m.score.sr_row_cap = 0;
        HIP_TRY(m.grow_scratch(grown, 1u, {{(void **)&m.score.d_sr_xs, (size_t)q_cap * cols * 4}, {(void **)&m.score.d_sr_rows, (size_t)q_cap * r_cap * 4},
                                           {(void **)&m.score.d_sr_scores, (size_t)q_cap * r_cap * 4}}));
        m.score.sr_q_cap = q_cap;
        m.score.sr_row_cap = r_cap;
    }
    // chunks of queries, and of list entries inside them: vectors and ids up, the launch, wait, scores down.
    for (int32_t q0 = 0; q0 < count; q0 += (int32_t)m.score.sr_q_cap) {
        const int32_t qc = std::min<int32_t>((int32_t)m.score.sr_q_cap, count - q0);
        if (host_xs) HIP_TRY(hipMemcpy(m.score.d_sr_xs, host_xs + (size_t)q0 * cols, (size_t)qc * cols * 4, hipMemcpyHostToDevice));
        for (int32_t r0 = 0; r0 < n_rows; r0 += (int32_t)m.score.sr_row_cap) {
            const int32_t rc = std::min<int32_t>((int32_t)m.score.sr_row_cap, n_rows - r0);
            if (rows_stride == 0)
                HIP_TRY(hipMemcpy(m.score.d_sr_rows, host_rows + r0, (size_t)rc * 4, hipMemcpyHostToDevice));
            else
                HIP_TRY(hipMemcpy2D(m.score.d_sr_rows, (size_t)rc * 4, host_rows + (size_t)q0 * (size_t)rows_stride + r0, (size_t)rows_stride * 4, (size_t)rc * 4,
                                    (size_t)qc, hipMemcpyHostToDevice));
            HIP_TRY(m.launch_and_wait([&] {
                m.launch_score_rows(host_xs ? m.score.d_sr_xs : installed, qc, m.score.d_sr_rows, rc, rows_stride == 0 ? 0u : (size_t)rc, m.score.d_sr_scores, m.stream);
            }));
            HIP_TRY(hipMemcpy2D(host_scores + (size_t)q0 * n_rows + r0, (size_t)n_rows * 4, m.score.d_sr_scores, (size_t)rc * 4, (size_t)rc * 4, (size_t)qc,
                                hipMemcpyDeviceToHost));
        }
    }
    return TKSPMV_OK;
}

int Engine::enqueue_row_stats(int32_t kind, float *dev_out, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_row_stats(m, "enqueue_row_stats", dev_out, kind, err)) return st;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_row_stats(kind, dev_out, s);
        return TKSPMV_OK;
    });
}

int Engine::row_stats(int32_t kind, float *host_out, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_row_stats(m, "row_stats", host_out, kind, err)) return st;
    if (m.desc.rows == 0u) return TKSPMV_OK;
    HIP_TRY(hipSetDevice(m.device));
    if (!m.stats.d_rs_out) HIP_TRY(m.alloc(m.stats.d_rs_out, (size_t)m.desc.rows * 4));
    HIP_TRY(m.launch_and_wait([&] { m.launch_row_stats(kind, m.stats.d_rs_out, m.stream); }));
    HIP_TRY(hipMemcpy(host_out, m.stats.d_rs_out, (size_t)m.desc.rows * 4, hipMemcpyDeviceToHost));
    return TKSPMV_OK;
}

int Engine::enqueue_assign(const float *dev_xs, int32_t count, uint32_t *dev_labels, float *dev_best, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_assign(m, "enqueue_assign", dev_xs, dev_labels, count, err)) return st;
    // (the launches behind the first merge with the scores of the ones before: without dev_best there is nowhere to keep them -- the
    //  engine owns no scratch that a call on a caller's stream could use without a wait)
    if (!dev_best && count > m.assign_pass())
        return fail(err, TKSPMV_ERR_INVALID, "dev_best = NULL takes one pass: count must not exceed the vectors of one pass (16384 / the column tier: 16, 4 or 1)");
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_assign(dev_xs, count, 0u, dev_labels, dev_best, s);
        return TKSPMV_OK;
    });
}

int Engine::assign(const float *host_xs, int32_t count, uint32_t *host_labels, float *host_best, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_assign(m, "assign", host_xs, host_labels, count, err)) return st;
    return m.assign_host(host_xs, count, 1u, host_labels, host_best, err, [&](const float *xs, int qc, uint32_t q0, uint32_t *labels, float *best) {
        m.launch_assign(xs, qc, q0, labels, best, m.stream);
    });
}

int Engine::enqueue_nearest(const float *dev_xs, int32_t count, int32_t n, const uint32_t *dev_mask, uint32_t *dev_labels, float *dev_scores, void *stream,
                            std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_nearest(m, "enqueue_nearest", dev_xs, dev_labels, dev_scores, false, count, n, dev_mask != nullptr, err)) return st;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_nearest(dev_xs, count, 0u, (uint32_t)count, (uint32_t)n, dev_mask, dev_labels, dev_scores, s);
        return TKSPMV_OK;
    });
}

int Engine::nearest(const float *host_xs, int32_t count, int32_t n, int32_t use_filter, uint32_t *host_labels, float *host_scores, std::string &err) {
    EngineImpl &m = *impl_;
    if (const int st = check_nearest(m, "nearest", host_xs, host_labels, host_scores, true, count, n, use_filter != 0, err)) return st;
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err, TKSPMV_ERR_STATE)) return st;
    return m.assign_host(host_xs, count, (uint32_t)n, host_labels, host_scores, err, [&](const float *xs, int qc, uint32_t q0, uint32_t *labels, float *scores) {
        m.launch_nearest(xs, qc, q0, (uint32_t)count, (uint32_t)n, mask, labels, scores, m.stream);
    });
}

int Engine::enqueue_label_sums(const uint32_t *dev_labels, uint32_t n_bins, int32_t quantum_exp, uint32_t flags, int64_t *dev_sums, int32_t mode, float *dev_out,
                               void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    constexpr uint32_t SINKS = TKSPMV_SUMS_SINK_LDS | TKSPMV_SUMS_SINK_DIRECT;
    if (!dev_sums || (reinterpret_cast<uintptr_t>(dev_sums) & 7u) != 0u || (dev_labels != nullptr) != (n_bins != 0u) || n_bins > (1u << 30) ||
        mode < TKSPMV_SUMS_RAW || mode > TKSPMV_SUMS_UNIT || (mode != TKSPMV_SUMS_RAW && !dev_out) || (flags & ~(TKSPMV_SUMS_ACCUMULATE | SINKS)) != 0u ||
        (flags & SINKS) == SINKS)
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_label_sums (dev_sums given and 8-byte aligned, dev_labels with 1 <= n_bins <= 2^30 or dev_labels = "
                                             "NULL with n_bins = 0, mode = TKSPMV_SUMS_RAW .. TKSPMV_SUMS_UNIT, dev_out given unless RAW, known flags, at most one sink)");
    if (const int st = m.row_scope(err, EngineImpl::SUMS_SCOPE)) return st;
    if (!dev_labels) {
        if (!m.grouped.have_groups) return fail(err, TKSPMV_ERR_INVALID, "no labels given and none installed (call tkspmv_set_groups first)");
        dev_labels = m.grouped.d_groups;
        n_bins = m.grouped.n_groups;
    }
    if ((flags & TKSPMV_SUMS_SINK_LDS) && !m.kern.label_sums[1])
        return fail(err, TKSPMV_ERR_INVALID, "TKSPMV_SUMS_SINK_LDS: the 16384-column tier has the direct sink only");
    const bool lds = (flags & SINKS) ? (flags & TKSPMV_SUMS_SINK_LDS) != 0u : m.label_sums_lds_sink(n_bins);
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_label_sums(dev_labels, n_bins, quantum_exp, (flags & TKSPMV_SUMS_ACCUMULATE) != 0u, lds, dev_sums, s);
        if (mode != TKSPMV_SUMS_RAW) m.launch_sums_close(dev_sums, n_bins, quantum_exp, mode, dev_out, s);
        return TKSPMV_OK;
    });
}

int Engine::enqueue_sums_close(const int64_t *dev_sums, uint32_t n_bins, int32_t quantum_exp, int32_t mode, float *dev_out, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_sums || (reinterpret_cast<uintptr_t>(dev_sums) & 7u) != 0u || !dev_out || n_bins < 1u || n_bins > (1u << 30) ||
        (mode != TKSPMV_SUMS_FLOAT && mode != TKSPMV_SUMS_UNIT))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_sums_close (dev_sums given and 8-byte aligned, dev_out given, 1 <= n_bins <= 2^30, mode = "
                                             "TKSPMV_SUMS_FLOAT or TKSPMV_SUMS_UNIT)");
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_sums_close(dev_sums, n_bins, quantum_exp, mode, dev_out, s);
        return TKSPMV_OK;
    });
}

int Engine::sums_exponent(int32_t *quantum_exp, std::string &err) {
    EngineImpl &m = *impl_;
    if (!quantum_exp) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to sums_exponent (output given)");
    if (const int st = m.row_scope(err, EngineImpl::SUMS_SCOPE)) return st;
    const size_t cols = m.desc.cols;
    std::vector<uint32_t> nnz(cols), hi(cols), lo(cols);
    if (const int st = col_stats(TKSPMV_COL_NNZ, 0, nnz.data(), err)) return st;
    if (const int st = col_stats(TKSPMV_COL_MAX, 0, hi.data(), err)) return st;
    if (const int st = col_stats(TKSPMV_COL_MIN, 0, lo.data(), err)) return st;
    *quantum_exp = sums_exponent_of_columns(nnz.data(), hi.data(), lo.data(), cols);
    return TKSPMV_OK;
}

int Engine::label_sums(const uint32_t *host_labels, uint32_t n_bins, int32_t quantum_exp, int32_t mode, int64_t *host_sums, float *host_out, std::string &err) {
    EngineImpl &m = *impl_;
    if ((host_labels != nullptr) != (n_bins != 0u) || n_bins > (1u << 30) || mode < TKSPMV_SUMS_RAW || mode > TKSPMV_SUMS_UNIT || (mode != TKSPMV_SUMS_RAW && !host_out))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to label_sums (host_labels with 1 <= n_bins <= 2^30 or host_labels = NULL with n_bins = 0, mode = "
                                             "TKSPMV_SUMS_RAW .. TKSPMV_SUMS_UNIT, host_out given unless RAW)");
    if (const int st = m.row_scope(err, EngineImpl::SUMS_SCOPE)) return st;
    if (!host_labels) {
        if (!m.grouped.have_groups) return fail(err, TKSPMV_ERR_INVALID, "no labels given and none installed (call tkspmv_set_groups first)");
        n_bins = m.grouped.n_groups;
    }
    HIP_TRY(hipSetDevice(m.device));
    EngineImpl::LabelSums &L = m.lsums;
    const size_t rows = m.desc.rows, cols = std::max<size_t>(m.desc.cols, 1), words = (size_t)n_bins * m.desc.cols;
    if (host_labels && !L.d_ls_labels) HIP_TRY(m.alloc(L.d_ls_labels, std::max<size_t>(rows, 1) * 4));
    if (n_bins > L.ls_cap) {
        HIP_TRY(hipStreamSynchronize(m.stream));  // (an earlier call's launches are long complete: label_sums waits itself)
        HIP_TRY(m.grow_scratch(L.ls_cap, n_bins, {{(void **)&L.d_ls_sums, (size_t)n_bins * cols * 8}, {(void **)&L.d_ls_out, (size_t)n_bins * cols * 4}}));
    }
    if (host_labels && rows) HIP_TRY(hipMemcpy(L.d_ls_labels, host_labels, rows * 4, hipMemcpyHostToDevice));
    // (UNIT leaves a bin without a norm unwritten: such a bin keeps what the caller's array holds)
    if (mode == TKSPMV_SUMS_UNIT && words) HIP_TRY(hipMemcpy(L.d_ls_out, host_out, words * 4, hipMemcpyHostToDevice));
    // No result is read and no result buffer written, so the engine need not be settled: the wait is for this call's own launches.
    if (const int st = enqueue_label_sums(host_labels ? L.d_ls_labels : nullptr, host_labels ? n_bins : 0u, quantum_exp, 0u, L.d_ls_sums, mode, L.d_ls_out, nullptr, err))
        return st;
    HIP_TRY(hipStreamSynchronize(m.stream));
    if (host_sums && words) HIP_TRY(hipMemcpy(host_sums, L.d_ls_sums, words * 8, hipMemcpyDeviceToHost));
    if (mode != TKSPMV_SUMS_RAW && words) HIP_TRY(hipMemcpy(host_out, L.d_ls_out, words * 4, hipMemcpyDeviceToHost));
    return TKSPMV_OK;
}

int Engine::enqueue_col_stats(int32_t kind, int32_t count, const uint32_t *dev_mask, int64_t mask_stride_words, void *dev_out, int64_t out_stride_words,
                              void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_out || kind < TKSPMV_COL_NNZ || kind > TKSPMV_COL_MIN || count < 1 || (!dev_mask && count != 1) || mask_stride_words < 0 || out_stride_words < 0 ||
        (count > 1 && out_stride_words < (int64_t)m.desc.cols))
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to enqueue_col_stats (output given, kind = TKSPMV_COL_NNZ .. TKSPMV_COL_MIN, count >= 1, count = 1 without "
                                             "masks, strides >= 0, out_stride_words >= cols with count > 1)");
    if (const char *why = m.col_stats_unsupported(dev_mask != nullptr)) return fail(err, TKSPMV_ERR_UNSUPPORTED, std::string("column statistics: ") + why);
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {  // (no result pair is written)
        m.launch_col_stats(kind, count, dev_mask, m.stride_of(dev_mask, mask_stride_words), static_cast<uint32_t *>(dev_out), (size_t)out_stride_words, s);
        return TKSPMV_OK;
    });
}

int Engine::col_stats(int32_t kind, int32_t use_filter, void *host_out, std::string &err) {
    EngineImpl &m = *impl_;
    if (!host_out || kind < TKSPMV_COL_NNZ || kind > TKSPMV_COL_MIN)
        return fail(err, TKSPMV_ERR_INVALID, "bad arguments to col_stats (output given, kind = TKSPMV_COL_NNZ .. TKSPMV_COL_MIN)");
    if (const char *why = m.col_stats_unsupported(use_filter != 0)) return fail(err, TKSPMV_ERR_UNSUPPORTED, std::string("column statistics: ") + why);
    const uint32_t *mask = nullptr;
    if (const int st = m.installed_mask(use_filter, mask, err, TKSPMV_ERR_STATE)) return st;
    if (m.desc.cols == 0u) return TKSPMV_OK;
    HIP_TRY(hipSetDevice(m.device));
    if (!m.cstats.d_cs_out) HIP_TRY(m.alloc(m.cstats.d_cs_out, (size_t)m.desc.cols * 4));
    HIP_TRY(m.launch_and_wait([&] { m.launch_col_stats(kind, 1, mask, 0u, m.cstats.d_cs_out, 0u, m.stream); }));
    HIP_TRY(hipMemcpy(host_out, m.cstats.d_cs_out, (size_t)m.desc.cols * 4, hipMemcpyDeviceToHost));
    return TKSPMV_OK;
}

int Engine::set_boost_cosine(std::string &err) {
    EngineImpl &m = *impl_;
    EngineImpl::Boost &Q = m.boost;
    if (const int st = m.row_scope(err, EngineImpl::STATS_SCOPE)) return st;
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(hipStreamSynchronize(m.stream));  // (a boosted query enqueued earlier may still read the installed arrays)
    Q.have_weight = Q.have_bias = false;  // (until the launch below has completed; the state aimed at is set_boost(w, NULL)'s)
    if (!Q.d_weight) HIP_TRY(m.alloc(Q.d_weight, std::max<size_t>(m.desc.rows, 1) * 4));
    // (the weights never visit the host; finite by construction)
    HIP_TRY(m.launch_and_wait([&] { m.launch_row_stats(TKSPMV_ROW_INV_L2, Q.d_weight, m.stream); }));
    Q.have_weight = true;
    return TKSPMV_OK;
}

int Engine::time_multi(const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || n_x < 1 || iters < 1 || !ns_per_query) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to time_multi");
    HIP_TRY(hipSetDevice(m.device));
    if (const int st = m.wait_idle(err)) return st;
    float ms = 0;
    const int timed = m.bracket_ms(ms, err, [&] {
        SequenceLists L(m, dev_xs, n_x, iters);
        if (m.multi.d_multi_out_idx) {  // a result buffer per query in flight (two groups): the two chains may run
            for (int i = 0; i < iters; ++i) {
                const size_t slot = (size_t)(i % (2 * MULTI_Q_MAX)) * (size_t)m.desc.k;
                L.oi[i] = m.multi.d_multi_out_idx + slot;
                L.ov[i] = m.multi.d_multi_out_val + slot;
            }
        }
        m.launch_multi_sequence(L.xs.data(), L.oi.data(), L.ov.data(), iters, m.stream);
    });
    if (timed != TKSPMV_OK) return timed;
    *ns_per_query = (double)ms * 1e6 / iters;
    if (m.diag.collect_stats) {  // TKSPMV_STATS=1: candidate-path counters of the multi-query kernel, per query
        unsigned long long st[32];
        HIP_TRY(hipMemcpy(st, m.diag.d_stats, sizeof(st), hipMemcpyDeviceToHost));
        const double n = (double)iters;
        fprintf(stderr, "[tkspmv multi stats per query] judged slices: offers %.1f rows %.1f (tau<=0: %.1f) overflowed %.1f | held slices: offers %.1f rows %.1f "
                        "(tau<=0: %.1f) overflowed %.1f | waits %.1f, %.2f us each\n",
                st[4] / n, st[5] / n, st[6] / n, st[7] / n, st[8] / n, st[9] / n, st[10] / n, st[11] / n, st[12] / n,
                st[12] ? st[13] * 0.01 / st[12] : 0.0);
        // (kept for tkspmv_debug_counters: the guard of the passes' threshold exchange is a COUNT -- waves that ran into their
        //  bounded wait, rows that overflowed a list -- not a wall clock)
        m.multi.multi_stat_queries += (uint64_t)iters;
        m.multi.multi_waits += st[12];
        m.multi.multi_wait_ticks += st[13];
        m.multi.multi_rows_offered += st[5] + st[9];
        m.multi.multi_rows_overflowed += st[7] + st[11];
        HIP_TRY(hipMemset(m.diag.d_stats, 0, 32 * 8));
    }
    m.host.result_on_device();
    return TKSPMV_OK;
}

int Engine::enqueue_deferred(const float *dev_x, uint32_t *dev_idx, float *dev_val, void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_x) return fail(err, TKSPMV_ERR_INVALID, "query vector is NULL");
    return enqueue_on(m, stream, true, err, [&](hipStream_t s) -> int {
        m.launch_deferred(dev_x, dev_idx ? dev_idx : m.host.d_out_idx, dev_val ? dev_val : m.host.d_out_val, s);
        return TKSPMV_OK;
    });
}

int Engine::drain(void *stream, std::string &err) {
    EngineImpl &m = *impl_;
    return enqueue_on(m, stream, false, err, [&](hipStream_t s) -> int {
        m.drain(s);
        return TKSPMV_OK;
    });
}

int Engine::run(double *kernel_ns, std::string &err) {
    EngineImpl &m = *impl_;
    if (!m.host.have_query) return fail(err, TKSPMV_ERR_STATE, "no query vector installed (call tkspmv_set_query first)");
    HIP_TRY(hipSetDevice(m.device));
    // The fused single launch can hand its result to the host itself (see h_res); the other launch schemes (radix select,
    // row per lane, unfused selection) complete in stream order and are waited for with the event.
    const bool to_host = m.host.host_path && m.host.h_res && m.defer.fused && !m.radix.use_radix && !(m.desc.impl == TKSPMV_IMPL_ROW_PER_LANE && m.multi.can_multi);
    const bool events = kernel_ns && (m.host.run_events || !to_host);
    const auto t_host0 = std::chrono::steady_clock::now();
    if (events) HIP_TRY(hipEventRecord(m.ev0, m.stream));
    // The result flag of the launch with the current epoch, polled (never longer than 2 s), and the block behind it verified.
    auto wait_flag = [&]() -> bool {
        volatile uint32_t *flag = m.host.h_res + 2 * (size_t)m.desc.k;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t spins = 0;; ++spins) {
            if (*flag == m.host.host_epoch && m.result_block_complete(m.host.host_epoch)) return true;
            __builtin_ia32_pause();
            if ((spins & 0xFFFFu) == 0xFFFFu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return false;
        }
    };
    bool seen = false;
    double own_ticks = 0.0;  // the launches' own durations (100 MHz ticks: first workgroup's entry -> result flag)
    if (to_host) {
        m.drain(m.stream);
        if (m.single.can_single) {
            // workgroup-local thresholds, checked by the selection (kernels/local.hpp); a failed check -- a query unlike the ones
            // before it -- sends the query through the exact launch below
            m.launch_single(m.host.d_x_cur, m.host.d_out_idx, m.host.d_out_val, m.stream, true);
            HIP_TRY(hipGetLastError());
            seen = wait_flag();
            if (seen) own_ticks += (double)m.host.h_res[2 * (size_t)m.desc.k + 1];
        }
        if (!m.single.can_single || !seen || m.host.h_res[2 * (size_t)m.desc.k + 5] != 0u) {
            if (m.single.can_single) ++m.single.single_repairs;
            m.host.h_res[2 * (size_t)m.desc.k + 5] = 0u;  // (only single_kernel writes the status word: the exact launch's block has none)
            m.launch_stream(m.host.d_x_cur, m.host.d_out_idx, m.host.d_out_val, m.stream, true);
            HIP_TRY(hipGetLastError());
            seen = wait_flag();
            if (seen) own_ticks += (double)m.host.h_res[2 * (size_t)m.desc.k + 1];
        }
    } else {
        m.launch_query(m.host.d_x_cur, m.host.d_out_idx, m.host.d_out_val, m.stream);
    }
    HIP_TRY(hipGetLastError());
    if (events) HIP_TRY(hipEventRecord(m.ev1, m.stream));
    if (!seen) HIP_TRY(hipStreamSynchronize(m.stream));
    HIP_TRY(m.settle());
    m.host.x_pending = false;  // the kernel has read x: the staging copy is free again
    if (kernel_ns && !events) {
        // the kernels' own durations, or the host clock if the flag never came
        if (seen) *kernel_ns = own_ticks * 10.0;
        else *kernel_ns = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_host0).count();
    }
    if (events) {
        if (seen) {  // the kernel is in its last instructions: the end event follows within a microsecond or two
            hipError_t q;
            while ((q = hipEventQuery(m.ev1)) == hipErrorNotReady) __builtin_ia32_pause();
            if (q != hipSuccess) return fail(err, TKSPMV_ERR_DEVICE, std::string("hipEventQuery failed: ") + hipGetErrorString(q));
        }
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, m.ev0, m.ev1));
        *kernel_ns = (double)ms * 1e6;
    }
    m.host.ran = true;
    m.host.last_on_host = seen;
    return TKSPMV_OK;
}

int Engine::synchronize(std::string &err) {
    HIP_TRY(hipSetDevice(impl_->device));
    impl_->drain(impl_->stream);
    return impl_->wait_idle(err);
}

int Engine::read(uint32_t *idx, float *val, int32_t *n, std::string &err) {
    EngineImpl &m = *impl_;
    if (!m.host.ran) return fail(err, TKSPMV_ERR_STATE, "no query has been run");
    if (m.host.last_on_host) {  // tkspmv_run left the result in pinned host memory
        if (idx) std::memcpy(idx, m.host.h_res, (size_t)m.desc.k * 4);
        if (val) std::memcpy(val, m.host.h_res + m.desc.k, (size_t)m.desc.k * 4);
        if (n) *n = m.desc.k;
        return TKSPMV_OK;
    }
    HIP_TRY(hipSetDevice(m.device));
    if (const int st = m.wait_idle(err)) return st;
    m.host.x_pending = false;
    if (idx) HIP_TRY(hipMemcpy(idx, m.host.d_out_idx, (size_t)m.desc.k * 4, hipMemcpyDeviceToHost));
    if (val) HIP_TRY(hipMemcpy(val, m.host.d_out_val, (size_t)m.desc.k * 4, hipMemcpyDeviceToHost));
    if (n) *n = m.desc.k;
    return TKSPMV_OK;
}

// out[0] = selections whose threshold check failed so far (each sent its query through the repair launch), out[1] = the current
// suspension length of carried thresholds, out[2] = selections to go until they are used again, out[3] = batch launches so far,
// out[4] = launches the local thresholds as a whole stay switched off for, out[5] = the length of that closure.
int Engine::debug_counters(unsigned long long *out, int n, std::string &err) {
    EngineImpl &m = *impl_;
    if (!out || n < 6) return fail(err, TKSPMV_ERR_INVALID, "debug_counters needs room for 6 values");
    HIP_TRY(hipSetDevice(m.device));
    if (const int st = m.wait_idle(err)) return st;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (m.local.d_wg_prior) HIP_TRY(hipMemcpy(w, m.local.d_wg_prior + m.grid, sizeof(w), hipMemcpyDeviceToHost));
    out[0] = w[3];
    out[1] = w[1];
    out[2] = w[0];
    out[3] = m.batch.batch_launches;
    out[4] = w[(m.batch.batch_launches & 1u) ? 7 : 4];  // launches the gate of the local thresholds stays closed for (the next launch's copy)
    out[5] = w[5];  // length of its latest closure
    if (n >= 10) {  // tkspmv_run through single_kernel: launches, queries sent on through the exact launch, failed checks, suspension
        uint32_t s[4] = {0, 0, 0, 0};
        if (m.single.d_lprior) HIP_TRY(hipMemcpy(s, m.single.d_lprior + m.grid, sizeof(s), hipMemcpyDeviceToHost));
        out[6] = m.single.single_launches;
        out[7] = m.single.single_repairs;
        out[8] = s[3];
        out[9] = s[0];
    }
    if (n >= 12) {  // round 5: batch launches that went out without a repair launch behind them, and the late repairs they cost
        out[10] = m.trust.trusted_launches;
        out[11] = m.trust.late_repairs;
    }
    if (n >= 14) {  // the pacing in force: quantum | levels << 8 | base << 16, and what tkspmv_create's measurement of it took (us; 0: not measured)
        out[12] = m.local.pace_quads | (m.local.pace_levels << 8) | (m.local.pace_base << 16) | ((uint64_t)m.local.pace_period_ns << 32);  // (upper half: the timetable's period, ns per query; 0: pauses by rank)
        out[13] = m.local.pace_tuned_us | ((uint64_t)m.local.pace_tune_launches << 32);  // (upper half: the batch launches the measurement made)
    }
    if (n >= 19) {  // option STATS, summed over the tkspmv_time_multi calls so far: queries, bounded waits for a threshold (count, ticks of 10 ns), rows offered / overflowed
        out[14] = m.multi.multi_stat_queries;
        out[15] = m.multi.multi_waits;
        out[16] = m.multi.multi_wait_ticks;
        out[17] = m.multi.multi_rows_offered;
        out[18] = m.multi.multi_rows_overflowed;
    }
    return TKSPMV_OK;
}

int Engine::read_trace(unsigned long long *host, size_t max_words, size_t *words, std::string &err) {
    EngineImpl &m = *impl_;
    if (!m.diag.d_trace && m.diag.d_wg_times) {  // option WG_TIMES: [BATCH_MAX + 1][grid] hand-over stamps of the last batch launch
        HIP_TRY(hipSetDevice(m.device));
        HIP_TRY(hipDeviceSynchronize());
        const size_t n = std::min(max_words, (size_t)(BATCH_MAX + 1) * m.grid);
        HIP_TRY(hipMemcpy(host, m.diag.d_wg_times, n * 8, hipMemcpyDeviceToHost));
        if (words) *words = n;
        return TKSPMV_OK;
    }
    if (!m.diag.d_trace) return fail(err, TKSPMV_ERR_STATE, "tracing is off (set TKSPMV_TRACE=1 before tkspmv_create)");
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = std::min(max_words, m.diag.trace_words * 4);
    HIP_TRY(hipMemcpy(host, m.diag.d_trace, n * 8, hipMemcpyDeviceToHost));
    if (words) *words = n;
    return TKSPMV_OK;
}

int Engine::result_device(const uint32_t **dev_idx, const float **dev_val) {
    if (dev_idx) *dev_idx = impl_->host.d_out_idx;
    if (dev_val) *dev_val = impl_->host.d_out_val;
    return TKSPMV_OK;
}

int Engine::scores(float *host_y, std::string &err) {
    EngineImpl &m = *impl_;
    if (!m.host.have_query) return fail(err, TKSPMV_ERR_STATE, "no query vector installed");
    HIP_TRY(hipSetDevice(m.device));
    if (!m.diag.d_scores) HIP_TRY(m.alloc(m.diag.d_scores, std::max<size_t>(m.desc.rows, 1) * 4));
    HIP_TRY(hipMemsetAsync(m.diag.d_scores, 0, std::max<size_t>(m.desc.rows, 1) * 4, m.stream));
    m.launch_scores(m.host.d_x_cur, m.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_y, m.diag.d_scores, (size_t)m.desc.rows * 4, hipMemcpyDeviceToHost, m.stream));
    if (const int st = m.wait_idle(err)) return st;
    return TKSPMV_OK;
}

int Engine::time_queries(const float *dev_xs, int32_t n_x, int32_t iters, double *ns_per_query, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || n_x < 1 || iters < 1 || !ns_per_query) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to time_queries");
    const bool host_times = opt("HOST_TIMES") != nullptr;  // (diagnostic: where the host's microseconds around the region go, to stderr)
    auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double h0 = host_times ? now_us() : 0.0;
    HIP_TRY(hipSetDevice(m.device));
    HIP_TRY(hipStreamSynchronize(m.stream));
    const double h1 = host_times ? now_us() : 0.0;
    // (batch launches on one stream: the bracket's events travel with the first and the last kernel; any other path records them)
    const int ext_mode = (int)opt_int("EXT_EVENTS", 1);
    const bool ext = m.batch.can_batch && ext_mode != 0;
    m.batch.ext_record = ext && ext_mode == 2;
    if (ext) {
        m.batch.ext_start = m.ev0;
        m.batch.ext_stop = m.ev1;
    } else {
        HIP_TRY(hipEventRecord(m.ev0, m.stream));
    }
    {
        const SequenceLists L(m, dev_xs, n_x, iters);
        m.launch_sequence(L.xs.data(), L.oi.data(), L.ov.data(), iters, m.stream);
    }
    if (!ext) HIP_TRY(hipEventRecord(m.ev1, m.stream));
    const double h2 = host_times ? now_us() : 0.0;
    if (m.batch.ext_start || m.batch.ext_stop) {  // (cannot happen: every batch path launches through launch_batch)
        m.batch.ext_start = m.batch.ext_stop = nullptr;
        err = "time_queries: the region's events were not attached to its launches";
        return TKSPMV_ERR_STATE;
    }
    // (polled: a blocking wait adds 10-20 us of wake-up latency to a region that may be as short as 400 us)
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(m.ev1);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIP_TRY(q);
        if (spins > (1u << 22)) {  // seconds of polling: something is wrong, let the runtime wait
            HIP_TRY(hipEventSynchronize(m.ev1));
            break;
        }
    }
    const double h3 = host_times ? now_us() : 0.0;
    HIP_TRY(m.settle());  // (the end event has passed: the stream is idle; a flagged query is repaired outside the event bracket)
    const double h4 = host_times ? now_us() : 0.0;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, m.ev0, m.ev1));
    if (host_times)
        fprintf(stderr, "[tkspmv] time_queries(%d): entry + wait for the idle stream %.1f us, lists + launches %.1f, until the end event is seen %.1f (the region itself %.1f), verdicts %.1f, elapsed time %.1f\n",
                iters, h1 - h0, h2 - h1, h3 - h2, (double)ms * 1e3, h4 - h3, now_us() - h4);
    *ns_per_query = (double)ms * 1e6 / iters;
    m.host.result_on_device();
    return TKSPMV_OK;
}

// `reps` repetitions of `iters` back-to-back queries, ALL enqueued before the first wait, one hipEvent between consecutive
// repetitions: ns_per_query[r] = the r-th repetition's time / iters. The GPU never idles between repetitions, so the figures
// are the kernel's under sustained load -- what tkspmv_time_queries measures when it is called in a loop is the kernel right
// after a host-side gap, 10-25 % slower for about a millisecond (power management: DESIGN.md).
int Engine::time_query_batches(const float *dev_xs, int32_t n_x, int32_t iters, int32_t reps, double *ns_per_query, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || n_x < 1 || iters < 1 || reps < 1 || reps > 4096 || !ns_per_query) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to time_query_batches");
    HIP_TRY(hipSetDevice(m.device));
    if (const int st = m.wait_idle(err)) return st;
    ScratchEvents scratch_events((size_t)reps + 1);
    std::vector<hipEvent_t> &evs = scratch_events.e;
    for (auto &e : evs) HIP_TRY(hipEventCreate(&e));
    const SequenceLists L(m, dev_xs, n_x, iters);
    HIP_TRY(hipEventRecord(evs[0], m.stream));
    for (int r = 0; r < reps; ++r) {
        m.launch_sequence(L.xs.data(), L.oi.data(), L.ov.data(), iters, m.stream);
        HIP_TRY(hipEventRecord(evs[(size_t)r + 1], m.stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(evs[(size_t)reps]));
    HIP_TRY(m.settle());
    for (int r = 0; r < reps; ++r) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, evs[(size_t)r], evs[(size_t)r + 1]));
        ns_per_query[r] = (double)ms * 1e6 / iters;
    }
    m.host.result_on_device();
    return TKSPMV_OK;
}

int Engine::time_stream_read(int32_t passes, double *ns_per_pass, std::string &err) {
    EngineImpl &m = *impl_;
    if (passes < 1 || !ns_per_pass) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to time_stream_read");
    if (m.pm.n_packets == 0) {
        *ns_per_pass = 0.0;
        return TKSPMV_OK;
    }
    HIP_TRY(hipSetDevice(m.device));
    const uint32_t stream_block = m.block;  // the streaming waves of a workgroup (the server wave of a sequence launch aside)
    ReadProbeParams R{};
    R.n_replicas = m.mat.d_replicas.empty() ? 1u : (uint32_t)std::min<size_t>(m.mat.d_replicas.size(), 8);
    // (what the batch kernel reads: its compact copies where the engine keeps them, the 20-bytes-per-lane probe over 1280-byte packets
    //  -- the floor of THAT kernel; a caller that rates a pass by the canonical stream's bytes overstates by 1408 / 1280)
    const uint32_t probe_packet_bytes = m.mat.batch_packet_bytes(m.pm);
    for (uint32_t r = 0; r < 8u; ++r) R.replicas[r] = m.mat.batch_packets(r);
    R.part_first = m.mat.d_part_first;
    R.part_count = m.mat.d_part_count;
    R.n_parts = (uint32_t)m.pm.part_first.size();
    R.n_pass = (uint32_t)passes;
    R.map = (uint32_t)opt_int("READ_PROBE_MAP", 0);
    R.period = period_units((uint64_t)opt_int("READ_PROBE_PERIOD", 0, 0, 0x7FFFFFFF));  // ns per pass: the probe on a timetable
    ScratchBuffer<uint32_t> sink;
    const size_t n_end = (size_t)m.grid * 16;
    HIP_TRY(hipMalloc((void **)&sink.p, (size_t)m.grid * 16 * 4 + (size_t)(passes + 2) * 128 + n_end * 8));
    R.sink = sink.p;
    R.claim = sink.p + (size_t)m.grid * 16;
    const bool want_ends = opt("READ_PROBE_ENDS") != nullptr;  // (tuning runs: when did the waves of each XCD finish?)
    R.t_end = want_ends ? reinterpret_cast<unsigned long long *>(R.claim + (size_t)(passes + 2) * 32) : nullptr;
    void (*fn)(ReadProbeParams) = nullptr;
    switch (probe_packet_bytes / 64u) {
        case 22: fn = read_probe_kernel<22>; break;
        case 24: fn = read_probe_kernel<24>; break;
        case 48: fn = read_probe_kernel<48>; break;
        case 16: fn = read_probe_kernel<16>; break;
        case 20: fn = read_probe_kernel<20>; break;
        case 12: fn = read_probe_kernel<12>; break;
        default: break;
    }
    if (const char *f = opt("READ_PROBE")) {  // "depth,work" (tuning runs; fp32 packets only)
        int depth = 8, work = 0;
        sscanf(f, "%d,%d", &depth, &work);
        if (probe_packet_bytes == 1536u) {
#define RP(D, W) if (depth == D && work == W) fn = read_probe_kernel<24, D, W>;
            if (depth == 22) fn = read_probe_kernel<22, 8, 1>;  // what 1408-byte packets would cost, read out of this 1536-byte stream
            RP(3, -1) RP(3, -2) RP(4, -2) RP(2, 0) RP(3, 0) RP(4, 0) RP(6, 0) RP(12, 0) RP(16, 0)
            RP(3, 1) RP(3, 32) RP(3, 64) RP(3, 96) RP(3, 128) RP(4, 64) RP(4, 96) RP(6, 64) RP(6, 96) RP(8, 64) RP(8, 96) RP(8, 1)
#undef RP
        }
    }
    if (!fn) return fail(err, TKSPMV_ERR_UNSUPPORTED, "no read probe for this packet size");
    if (const int st = m.wait_idle(err)) return st;
    R.n_pass = 2;  // (warm-up: code object, clocks)
    HIP_TRY(hipMemsetAsync(R.claim, 0, (size_t)(passes + 2) * 128, m.stream));
    hipLaunchKernelGGL(fn, dim3(m.grid), dim3(stream_block), 0, m.stream, R);
    R.n_pass = (uint32_t)passes;
    HIP_TRY(hipMemsetAsync(R.claim, 0, (size_t)(passes + 2) * 128, m.stream));
    float ms = 0;
    if (const int st = m.bracket_ms(ms, err, [&] { hipLaunchKernelGGL(fn, dim3(m.grid), dim3(stream_block), 0, m.stream, R); })) return st;
    HIP_TRY(hipGetLastError());
    if (want_ends) {
        std::vector<unsigned long long> te(n_end);
        HIP_TRY(hipMemcpy(te.data(), R.t_end, n_end * 8, hipMemcpyDeviceToHost));
        const uint32_t nw = stream_block / 64u;
        unsigned long long t0 = ~0ull, t1 = 0ull;
        for (uint32_t b = 0; b < m.grid; ++b)
            for (uint32_t w = 0; w < nw; ++w) {
                t0 = std::min(t0, te[(size_t)b * nw + w]);
                t1 = std::max(t1, te[(size_t)b * nw + w]);
            }
        fprintf(stderr, "[read probe] wave end times relative to the last one, by blockIdx %% 8 (mean / earliest, us):");
        for (uint32_t x = 0; x < 8u; ++x) {
            double sum = 0, mn = 1e30;
            uint32_t n = 0;
            for (uint32_t b = x; b < m.grid; b += 8u)
                for (uint32_t w = 0; w < nw; ++w, ++n) {
                    const double d = (double)(t1 - te[(size_t)b * nw + w]) * 0.01;
                    sum += d;
                    mn = std::min(mn, -d);
                }
            fprintf(stderr, " %.1f / %.1f", -sum / std::max(1u, n), mn);
        }
        fprintf(stderr, "  (launch %.1f us)\n", (double)ms * 1e3);
        std::vector<double> lead;
        for (size_t i = 0; i < n_end; ++i)
            if (te[i] != 0ull && (double)(t1 - te[i]) * 0.01 < (double)ms * 1e3 * 0.9) lead.push_back((double)(t1 - te[i]) * 0.01);
        std::sort(lead.begin(), lead.end());
        if (!lead.empty()) {
            fprintf(stderr, "[read probe] waves still running x us before the end of the launch:");
            for (double x : {1.0, 5.0, 10.0, 20.0, 40.0, 80.0, 160.0, 320.0})
                fprintf(stderr, " %g us: %zu", x, (size_t)(std::lower_bound(lead.begin(), lead.end(), x) - lead.begin()));
            fprintf(stderr, " (of %zu)\n", lead.size());
        }
    }
    *ns_per_pass = (double)ms * 1e6 / passes;
    return TKSPMV_OK;
}

int Engine::profile(const float *dev_xs, int32_t n_x, int32_t iters, tkspmv_timing *out, std::string &err) {
    EngineImpl &m = *impl_;
    if (!dev_xs || n_x < 1 || iters < 1 || !out) return fail(err, TKSPMV_ERR_INVALID, "bad arguments to profile");
    std::memset(out, 0, sizeof(*out));
    HIP_TRY(hipSetDevice(m.device));
    if (const int st = m.wait_idle(err)) return st;
    unsigned long long st0[8], st1[8];
    HIP_TRY(hipMemcpy(st0, m.diag.d_stats, sizeof(st0), hipMemcpyDeviceToHost));
    const size_t stride = m.desc.cols;
    // (1) whole queries back-to-back
    float ms = 0;
    const int timed = m.bracket_ms(ms, err, [&] {
        const SequenceLists L(m, dev_xs, n_x, iters);
        m.launch_sequence(L.xs.data(), L.oi.data(), L.ov.data(), iters, m.stream);
    });
    if (timed != TKSPMV_OK) return timed;
    out->query_ns = (double)ms * 1e6 / iters;
    HIP_TRY(hipMemcpy(st1, m.diag.d_stats, sizeof(st1), hipMemcpyDeviceToHost));
    out->candidates_avg = (double)(st1[0] - st0[0]) / (double)std::max<unsigned long long>(1, st1[1] - st0[1]);
    out->slow_paths_avg = (double)(st1[4] - st0[4]) / (double)std::max<unsigned long long>(1, st1[1] - st0[1]);
    out->appended_avg = (double)(st1[5] - st0[5]) / (double)std::max<unsigned long long>(1, st1[1] - st0[1]);
    // (2) per-kernel: an event before and after every stream kernel, everything enqueued back to back and one
    // host sync at the end, so the GPU never idles between launches (an idle GPU adds the dispatch latency of the
    // next kernel to the interval).
    double t_stream = 0, t_select = 0;
    {
        ScratchEvents scratch_events((size_t)iters * 2 + 1);
        std::vector<hipEvent_t> &evs = scratch_events.e;
        for (auto &e : evs) HIP_TRY(hipEventCreate(&e));
        for (int i = 0; i < iters; ++i) {
            const float *x = dev_xs + (size_t)(i % n_x) * stride;
            HIP_TRY(hipEventRecord(evs[2 * i], m.stream));
            if (m.radix.use_radix) m.launch_query(x, m.host.d_out_idx, m.host.d_out_val, m.stream);  // (scores + radix select + selection)
            else if (m.single.can_single) m.launch_single(x, m.host.d_out_idx, m.host.d_out_val, m.stream, false);  // (what tkspmv_run launches)
            else m.launch_stream(x, m.host.d_out_idx, m.host.d_out_val, m.stream);
            HIP_TRY(hipEventRecord(evs[2 * i + 1], m.stream));
            if (!m.defer.fused && !m.radix.use_radix) m.launch_select(m.host.d_out_idx, m.host.d_out_val, m.stream);
        }
        HIP_TRY(hipEventRecord(evs[2 * iters], m.stream));
        HIP_TRY(hipEventSynchronize(evs[2 * iters]));
        for (int i = 0; i < iters; ++i) {
            float a = 0, b = 0;
            HIP_TRY(hipEventElapsedTime(&a, evs[2 * i], evs[2 * i + 1]));
            HIP_TRY(hipEventElapsedTime(&b, evs[2 * i + 1], evs[2 * i + 2]));
            t_stream += a;
            t_select += b;
        }
    }
    // (3) SpMV-only variant (hw_spmv_only_time of the reference's GPU host): full y written, no top-k
    {
        if (!m.diag.d_scores) HIP_TRY(m.alloc(m.diag.d_scores, std::max<size_t>(m.desc.rows, 1) * 4));
        float ms2 = 0;
        const int st = m.bracket_ms(ms2, err, [&] {
            for (int i = 0; i < iters; ++i) m.launch_scores(dev_xs + (size_t)(i % n_x) * stride, m.stream);
        });
        if (st != TKSPMV_OK) return st;
        out->scores_kernel_ns = (double)ms2 * 1e6 / iters;
    }
    // (4) what the event bracket itself costs around one launch: the same bracket around an empty kernel with
    // the same geometry, enqueued the same way (followed by the select kernel so the stream stays busy).
    double t_null = 0;
    {
        const int n = iters < 200 ? iters : 200;
        ScratchEvents scratch_events((size_t)n * 2);
        std::vector<hipEvent_t> &evs = scratch_events.e;
        for (auto &e : evs) HIP_TRY(hipEventCreate(&e));
        for (int i = 0; i < n; ++i) {
            HIP_TRY(hipEventRecord(evs[2 * i], m.stream));
            hipLaunchKernelGGL(null_kernel, dim3(m.grid), dim3(m.block + 64), 0, m.stream, m.ex.st[0].gmax);
            HIP_TRY(hipEventRecord(evs[2 * i + 1], m.stream));
            if (!m.defer.fused && !m.radix.use_radix) m.launch_select(m.host.d_out_idx, m.host.d_out_val, m.stream);
        }
        if (const int st = m.wait_idle(err)) return st;
        for (int i = 0; i < n; ++i) {
            float a = 0;
            HIP_TRY(hipEventElapsedTime(&a, evs[2 * i], evs[2 * i + 1]));
            t_null += a;
        }
        t_null = t_null * 1e6 / n;
    }
    out->event_bracket_ns = t_null;
    out->stream_kernel_ns = t_stream * 1e6 / iters;
    out->select_kernel_ns = t_select * 1e6 / iters;
    out->n_queries = (uint32_t)iters;
    if (m.diag.collect_stats) {
        unsigned long long sx[14];
        HIP_TRY(hipMemcpy(sx, m.diag.d_stats, sizeof(sx), hipMemcpyDeviceToHost));
        const double nsel = (double)std::max<unsigned long long>(1, sx[1]);
        fprintf(stderr, "[tkspmv stats] selections %llu, general-path selections %llu, max candidates %llu, overflow entries per selection %.1f; "
                        "per selection: waves that waited for a threshold at the end of their partition %.1f (%.1f us in all)\n",
                sx[1], sx[3], sx[2], (double)sx[8] / nsel, (double)sx[10] / nsel, (double)sx[9] / 100.0 / nsel);
    }
    if (m.diag.collect_stamps) {
        unsigned long long st[16];
        HIP_TRY(hipMemcpy(st, m.diag.d_stats + 16, sizeof(st), hipMemcpyDeviceToHost));
        fprintf(stderr, "[tkspmv stamps, shader cycles since stream end of the last workgroup] flush_issued %lld flush_done %lld ticket %lld loads %lld keys %lld ranked %lld end %lld\n",
                (long long)(st[1] - st[0]), (long long)(st[2] - st[0]), (long long)(st[3] - st[0]), (long long)(st[4] - st[0]),
                (long long)(st[5] - st[0]), (long long)(st[6] - st[0]), (long long)(st[7] - st[0]));
    }
    m.host.result_on_device();
    return TKSPMV_OK;
}

// The reference's loop -- reset(x) from host memory, operator(), read_result() (host_spmv_bscsr.cpp:602-632) -- `iters` times in
// native code, cycling over n_x host vectors: loop_ns[i] = the host's steady clock around the three calls of iteration i,
// kernel_ns[i] = what tkspmv_run returned for it. What a C++ host of the reference sees per iteration; a Python caller adds a
// ctypes transition per call to it.
int Engine::time_host_loop(const float *host_xs, int32_t n_x, int32_t iters, double *loop_ns, double *kernel_ns, std::string &err) {
    if (!host_xs || n_x < 1 || iters < 1 || !loop_ns) return fail(err, TKSPMV_ERR_INVALID, "time_host_loop: NULL or empty arguments");
    EngineImpl &m = *impl_;
    std::vector<uint32_t> idx((size_t)m.desc.k);
    std::vector<float> val((size_t)m.desc.k);
    for (int32_t i = 0; i < iters; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        double set_ns = 0.0, k_ns = 0.0;
        int32_t n = 0;
        int st = set_query(host_xs + (size_t)(i % n_x) * m.desc.cols, &set_ns, err);
        if (st == TKSPMV_OK) st = run(&k_ns, err);
        if (st == TKSPMV_OK) st = read(idx.data(), val.data(), &n, err);
        if (st != TKSPMV_OK) return st;
        loop_ns[i] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        if (kernel_ns) kernel_ns[i] = k_ns;
    }
    return TKSPMV_OK;
}

}  // namespace tkspmv
