// scvote.hip -- C ABI (include/scvote.h) over the gfx950 kernels in scvote_kernels.hip.h.
//
// Host-side responsibilities: argument validation, launch geometry (persistent grid sized from
// the CU count), variant dispatch for A/B tuning, hipEvent timing on the launch stream, and the
// HOST-memory staging path.  No C++ exception crosses the ABI; every entry returns 0 or a
// negative code and sets a thread-local message.
#define SCV_TU_MAIN 1   // the non-template kernels are emitted by this translation unit only
#include "scvote_kernels.hip.h"
#include "scvote_dispatch.h"
#include "scvote_plan.h"
#include "scvote_hostpool.h"
#include "scvote_expected_table.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <vector>

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// No C++ exception crosses the C ABI (include/scvote.h): every extern "C" body runs inside guarded().  What can throw
// on the host side is the standard library (std::vector / std::function growth: std::bad_alloc; std::thread creation in a container
// with a thread limit: std::system_error); all of it becomes an error code + message, never std::terminate in a ctypes caller.
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(SCV_ERR_ALLOC, "out of host memory (std::bad_alloc inside the library)");
    } catch (const std::exception& e) {
        return fail(SCV_ERR_ARG, "internal error: %s", e.what());
    } catch (...) {
        return fail(SCV_ERR_ARG, "internal error: unknown C++ exception");
    }
}

// TEST HOOK, compiled only with -DSCV_TEST_HOOKS (the `hooks` variant of _build.py: csrc/libscvote_hooks.so, which only
// tests/test_gpu_parity.py loads; libscvote.so, the product, never reads the environment): SCV_TEST_FAULT makes the HOST-mode staging
// path fail the way a starved container would -- "thread": every worker-thread creation raises std::system_error (the pipeline must
// run on the calling thread alone); "alloc": std::bad_alloc while the copy pieces are built; "throw": a std::runtime_error.
int test_fault() {
#ifdef SCV_TEST_HOOKS
    const char* f = getenv("SCV_TEST_FAULT");
    if (!f || !*f) return 0;
    if (!strcmp(f, "thread")) return 1;
    if (!strcmp(f, "alloc")) return 2;
    if (!strcmp(f, "throw")) return 3;
    if (!strcmp(f, "race")) return 4;          // a DELIBERATE data race among the copy pieces: proves that a sanitizer run would see one
#endif
    return 0;
}

#define SCV_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SCV_ERR_ALLOC : -(int)e_, "%s: %s", #expr,     \
                        hipGetErrorString(e_));                                                    \
    } while (0)

struct EventPair { hipEvent_t a, b; };

}  // namespace

// ---- HOST-mode ingestion pipeline -----------------------------------------------------
// Real (non-synthetic) answer tensors arrive in pageable host memory, and then the 63 GB/s PCIe link -- not HBM --
// bounds end-to-end votes/s.  A pageable hipMemcpyAsync goes through the runtime's own bounce buffers with one
// copying thread (measured 38-46 GB/s, and it blocks the host).  Here the chunk loop is a three-stage pipeline:
//   worker threads   memcpy chunk i+1 of the caller's buffers into a PINNED bounce slot   (several cores)
//   copy stream      DMA slot -> HBM slot of chunk i                                       (one 55+ GB/s transfer)
//   compute stream   hot-path kernel(s) on chunk i-1, cell table back to the caller
// with two bounce slots, two HBM slots and events between the stages.  Buffers the caller has already pinned
// (hipHostMalloc / hipHostRegister: scv_host_alloc) skip the bounce and are DMA'd in place.
struct HostPipe {
    static constexpr int kSlots = 2;
    hipStream_t copy_stream = nullptr;
    hipEvent_t landed[kSlots] = {nullptr, nullptr};      // H2D of the slot finished (bounce slot reusable, kernel may start)
    hipEvent_t consumed[kSlots] = {nullptr, nullptr};    // kernel + cell D2H on the slot finished (HBM slot reusable)
    void* bounce[kSlots] = {nullptr, nullptr};           // pinned host memory
    size_t bounce_bytes = 0;
    void* dslot[kSlots] = {nullptr, nullptr};            // HBM
    size_t dslot_bytes = 0;
    // worker threads for the pageable -> pinned copies: plain C++ with no HIP in it (scvote_hostpool.h), so that gcc's
    // -fsanitize=thread / address can be pointed at it on the CPU (tests/hostpool_sanitize.cpp)
    scv::CopyPool pool;
    void start(int nthreads, bool fail_for_test = false) noexcept { pool.start(nthreads, fail_for_test); }
    void run(std::vector<std::function<void()>>&& pieces) { pool.run(std::move(pieces)); }
    void shutdown() {
        pool.join_all();
        for (int k = 0; k < kSlots; ++k) {
            if (landed[k]) (void)hipEventDestroy(landed[k]);
            if (consumed[k]) (void)hipEventDestroy(consumed[k]);
            if (bounce[k]) (void)hipHostFree(bounce[k]);
            if (dslot[k]) (void)hipFree(dslot[k]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

struct scv_ctx {
    int device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    int64_t lds_max = 65536;
    int64_t clock_khz = 0;
    int64_t hbm_bytes = 0;
    // streaming-kernel geometry (scv_set_tuning; auto unless user_tuned)
    int copies = 16, threads = 1024, wg_per_cu = 1, unroll = 4;
    bool user_tuned = false; // set_tuning called: auto geometry off
    // options (scv_set_option; include/scvote.h documents every key)
    int path = 0;            // 0 auto | 1 streaming, whole cells | 2 streaming, split-N | 3 streaming, whole cells, round-robin items | 4 register-resident cells | 5 sorted cells
    int segs_override = 0;   // > 0: segments per cell for path 2
    int split_seg_kb = 256;  // split-N: smallest segment the auto choice cuts (KiB)
    int overwrite_counters = 0;  // DEVICE mode: per-budget outputs are overwritten instead of accumulated into (no caller memset)
    int sort_n_min = 8;      // sorted cells (scv_sort_cells): sort_n_min <= N <= sort_n_max (rows that are not 16-byte aligned: from 5); shorter
    int sort_n_max = 64;     // cells stay on scv_lane_cells, longer ones go to the register-resident kernels; sort_n_max = 0: off
    int reg_n_max = 8192;    // auto: 32 < N <= this -> register-resident cells (scv_reg_cells / scv_reg_dense); 0 = off (streaming kernel)
    int reg_shape = 0;       // force a register-resident shape (parity tests, A/B runs), see scvote_plan.h reg_shape
    int fused_counters_max = 512;   // cells: at or below, counters inside the hot kernel; above, scv_reduce_cells; 0: always the reduction.  (Round 6, tools/crossovers.py:
                                    // 4096 until then -- at 2048 / 4096 / 8192 cells of 64 KiB the per-cell atomics cost 41 / 73 / 138 us against 29 / 50 / 89 with the reduction;
                                    // equal at 512 cells, 4 % better at 256)
    int grid_override = 0;   // > 0: exact persistent grid size
    int prefix_path = 0;     // prefix budgets: 0 auto | 1 one lane per problem | 2 cell kernels on pool rows | 3 one-pass streaming snapshots |
                             // 4 one pass per problem, G lanes per problem (scv_prefix_pool; "reg_shape" 16 / 32 / 64 forces G)
    int boot_path = 0;       // vote + bootstrap: 0 auto (one cooperative launch when the shape allows) | 1 one ORDINARY launch | 2 two launches,
                             // LDS-resident code table | 3 two launches, global gathers
    int boot_spin_limit = 1 << 20;   // polls (x s_sleep 8) a workgroup waits at the grid barrier before giving up (tests force 1)
    int stage_mb = 128;      // HOST mode: chunk size (votes + tokens) of the staging pipeline
    int copy_threads = 6;    // HOST mode (4-8 reach the link rate; 16+ were unstable: 30-55 GB/s run to run): threads copying pageable caller memory
    // fixed choices that used to be options (measured: DESIGN_HISTORY.md 4 "dead ends")
    static constexpr int tiny_n_max = 32;   // N <= this (and below sort_n_min): one lane per cell, registers only (scv_lane_cells)
    void* d_tickets = nullptr;   // arrival counters of the single-launch modes (all zero between launches)
    size_t d_tickets_words = 0;
    int64_t stat_boot_fused = 0, stat_boot_separate = 0, stat_overwrite_fused = 0, stat_lds_counters = 0, stat_prefix_cells = 0, stat_prefix_lane = 0;   // scv_get_stat
    struct BootReq { int32_t r0, r1, M; uint64_t seed; int64_t* out; bool fused; }* boot_req = nullptr;   // set for the duration of one call
    // the last fused request, kept so that a grid-barrier timeout can be repaired at scv_sync by a separate bootstrap launch
    struct BootLast { const scv_cell* cells = nullptr; int64_t P = 0; int32_t B = 0, r0 = 0, r1 = 0, M = 0; uint64_t seed = 0; int64_t* out = nullptr; bool valid = false; } boot_last;
    int64_t stat_boot_recovered = 0, stat_boot_cooperative = 0, stat_sort_cells = 0, stat_few_votes = 0, stat_prefix_pool = 0;
    int64_t stat_prefix_sort = 0, stat_prefix_tokens = 0, stat_one_vote = 0;
    const int32_t* nv_host = nullptr;   // HOST-mode calls: the caller's n_valid (host memory) for the duration of the call -- launch_prefix reads the budgets
    // split-N scratch (grown on demand)
    void* d_partial = nullptr;
    size_t d_partial_bytes = 0;
    void* d_cells = nullptr;  // cell table scratch for the reduce kernel when the caller wants no cells
    size_t d_cells_bytes = 0;
    // device scratch
    uint32_t* d_err = nullptr;
    bool err_dirty = false;
    // timing
    std::vector<EventPair> events;
    size_t events_used = 0;
    // HOST-mode staging (grown on demand)
    void* d_stage = nullptr;
    size_t d_stage_bytes = 0;
    HostPipe* pipe = nullptr;       // HOST-mode ingestion pipeline (created on the first HOST call)
    // HOST-mode small calls (everything the reference itself asks for: P = 30, N <= 128, o1.py:277,302): one pinned block and one
    // HBM block owned by the ctx, allocated on the first small call
    void* small_h = nullptr;
    void* small_d = nullptr;
    size_t small_bytes = 0;
    int small_call_kb = 1024;       // option "host_small_kb": calls whose inputs + outputs fit in this many KiB take the small path (0: never)
    int64_t stat_small_calls = 0, stat_pipelined_calls = 0;
    int64_t stat_resample_calls = 0;    // scv_resample_prefix_i32 calls that launched the kernel
    int64_t stat_expected_calls = 0;    // scv_expected_majority_i32 launches
    int64_t stat_token_budget_calls = 0;    // scv_token_budget_prefix_i32 launches
    double* d_expected_tab = nullptr;   // scv::kExpectedTabWords: binomials and Gauss-Legendre points (written at scv_create)
};

namespace {

constexpr size_t kMaxTimedLaunches = 8192;   // timing ring: undrained records beyond this are dropped

// Next hipEvent pair of the timing ring (NULL without SCV_FLAG_TIMING).
int next_event_pair(scv_ctx* ctx, EventPair** out) {
    *out = nullptr;
    if (!(ctx->flags & SCV_FLAG_TIMING)) return SCV_OK;
    if (ctx->events_used >= kMaxTimedLaunches) ctx->events_used = 0;
    if (ctx->events_used == ctx->events.size()) {
        EventPair np;
        SCV_HIP(hipEventCreate(&np.a));
        SCV_HIP(hipEventCreate(&np.b));
        ctx->events.push_back(np);
    }
    *out = &ctx->events[ctx->events_used++];
    return SCV_OK;
}


// Kernel variant tables live in their own translation units (scvote_stream_*.hip, scvote_reg.hip, scvote_dense.hip):
// the template instantiations are compiled in parallel and only the table that changed is rebuilt (csrc/scvote_dispatch.h).
using scv::KernelFn;
using scv::RegKernel;
using scv::pick_kernel;
using scv::pick_reg_kernel;
using scv::pick_dense_kernel;
using scv::pick_sort_kernel;
using scv::pick_prefix_pool_kernel;
using scv::pick_sort_prefix_kernel;
using scv::pick_resample_kernel;

// Every entry point runs on the ctx device and leaves the caller's current HIP device as it found it
// (a process driving several GPUs from one thread -- MultiDeviceEngine -- must not have torch's
// current device moved under it).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int enter(int device) {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
        if (prev != device) {
            SCV_HIP(hipSetDevice(device));
            switched = true;
        }
        return SCV_OK;
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};
#define SCV_ENTER(ctx)                                                                             \
    DeviceGuard guard_;                                                                            \
    if (int rc_ = guard_.enter((ctx)->device)) return rc_

int ensure_cells(scv_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->d_cells_bytes) return SCV_OK;
    if (ctx->d_cells) { SCV_HIP(hipFree(ctx->d_cells)); ctx->d_cells = nullptr; ctx->d_cells_bytes = 0; }
    SCV_HIP(hipMalloc(&ctx->d_cells, bytes));
    ctx->d_cells_bytes = bytes;
    return SCV_OK;
}

// Arrival counters of the single-launch modes (overwrite-counters, vote + bootstrap): 4 words, zero when allocated at scv_create,
// and every counter is reset by the workgroup that completes it, so they are all-zero again whenever no launch is in flight.
// Nothing allocates on the launch path: legal inside hipGraph capture and independent of later scv_set_stream calls.
constexpr size_t kTicketWords = 8 + scv::kSplitTickets;     // [0 .. 2] the single-launch epilogues | [3] the dynamic-items dispenser | [8 + cell] split-N arrival counters

// split-N scratch: the split cells' histograms and token sums in memory.  All zero whenever no launch is in flight (the workgroup that
// finishes a cell clears what it read), so it is cleared here once, when it is (re)allocated -- ON THE CONTEXT'S STREAM: the stream is
// non-blocking, so a hipMemset (null stream, asynchronous to the host for device memory) is not ordered before the launch that follows and
// could clear sums the first segments had already added (round 6: fuzz seeds 116 / 155 -- calls in which the scratch grows -- failed in a test
// selection without a DEVICE-mode call in front; in the full suite such a call binds the context to torch's null stream early, which ordered the two:
// profiles/r06_split_scratch_race.log).
int ensure_partial(scv_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->d_partial_bytes) return SCV_OK;
    if (ctx->d_partial) { SCV_HIP(hipStreamSynchronize(ctx->stream)); SCV_HIP(hipFree(ctx->d_partial)); ctx->d_partial = nullptr; ctx->d_partial_bytes = 0; }
    SCV_HIP(hipMalloc(&ctx->d_partial, bytes));
    SCV_HIP(hipMemsetAsync(ctx->d_partial, 0, bytes, ctx->stream));
    ctx->d_partial_bytes = bytes;
    return SCV_OK;
}

// ---- the dense and prefix aggregate launches (scv_aggregate_i32, scv_aggregate_prefix_i32) -------------------------------------------------
// WHICH kernel, register shape, segment count and LDS size serve a call is decided in scvote_plan.h (plain C++, checked on the CPU by
// tests/test_dispatch_plan_cpu.py); this file asks the runtime what the plan needs to know (occupancy) and launches, one launcher per kind.
namespace plan = scv::plan;
static_assert(plan::kBins == scv::kBins && plan::kRedWords == scv::kRedWords && plan::kMaxSortedB == scv::kMaxSortedB &&
              plan::kSplitTickets == scv::kSplitTickets && plan::kCellBytes == sizeof(scv_cell), "scvote_plan.h restates these");

plan::Options plan_options(const scv_ctx* ctx) {
    return plan::Options{ctx->path, ctx->prefix_path, ctx->tiny_n_max, ctx->reg_n_max, ctx->sort_n_max, ctx->sort_n_min, ctx->reg_shape,
                         ctx->fused_counters_max, ctx->overwrite_counters, ctx->segs_override, ctx->split_seg_kb,
                         ctx->copies, ctx->threads, ctx->wg_per_cu, ctx->unroll, ctx->user_tuned, ctx->num_cus, ctx->lds_max};
}

// One call: the caller's pointers and shape, and what every launcher derives from them.
struct AggCall {
    const int32_t* answers; const int32_t* tokens; const int32_t* n_valid; const int32_t* truth;
    int64_t P; int32_t B; int64_t N;
    scv_cell* cells; int64_t* cell_tokens; int64_t* tie; int64_t* tok_sum; int64_t* truth_sum;
    int64_t ncells() const { return P * (int64_t)B; }
    bool tok() const { return tokens != nullptr; }
    bool want_counters() const { return tie || truth_sum || (tok() && tok_sum); }
    bool bases_aligned() const { return (((uintptr_t)answers & 15u) == 0) && (!tok() || ((uintptr_t)tokens & 15u) == 0); }
    bool rows_aligned() const { return (N % 4 == 0) && bases_aligned(); }
};

// The AggArgs fields every kernel of the two entries reads, from the call; the rest at their defaults (whole cells in descending n_valid
// order, counters accumulated into the caller's arrays, no prefetch, no single-launch epilogue).  A launcher sets only what differs.
scv::AggArgs agg_args(const scv_ctx* ctx, const AggCall& c) {
    scv::AggArgs a;
    a.answers = c.answers; a.tokens = c.tokens; a.n_valid = c.n_valid; a.truth = c.truth;
    a.ncells = c.ncells(); a.N = c.N; a.B = c.B; a.P = c.P;
    a.cells = c.cells; a.cell_tokens = c.tok() ? c.cell_tokens : nullptr;      // cell_tokens_out is written only by a call with tokens, in both memory modes
    a.tie_hits = reinterpret_cast<unsigned long long*>(c.tie);
    a.token_sum = reinterpret_cast<unsigned long long*>(c.tok_sum); a.truth_sum = reinterpret_cast<unsigned long long*>(c.truth_sum);
    a.err_flag = ctx->d_err;
    a.prefetch = 0; a.sorted = 1; a.pool_rows = 0;
    a.segs = 1; a.seg_len = c.N; a.partial = nullptr; a.partial_tok = nullptr; a.wave_lds_words = 0; a.acc_classes = 0;
    a.tickets = nullptr; a.overwrite = 0; a.ow_tie = a.ow_tok = a.ow_truth = nullptr;
    a.boot = 0; a.boot_r0 = a.boot_r1 = 0; a.boot_M = 1; a.boot_spins = 0; a.boot_seed = 0; a.boot_out = nullptr;
    return a;
}

// Overwrite semantics (option "overwrite_counters") for every launch that accumulates: memset nodes in front of it.
int clear_counters(scv_ctx* ctx, int64_t* tie, int64_t* tok_sum, int64_t* truth_sum, int32_t B) {
    if (tie) SCV_HIP(hipMemsetAsync(tie, 0, (size_t)B * SCV_TIE_CLASSES * sizeof(int64_t), ctx->stream));
    if (tok_sum) SCV_HIP(hipMemsetAsync(tok_sum, 0, (size_t)B * sizeof(int64_t), ctx->stream));
    if (truth_sum) SCV_HIP(hipMemsetAsync(truth_sum, 0, (size_t)B * sizeof(int64_t), ctx->stream));
    return SCV_OK;
}

// The counters will be computed from the cell table (scv_reduce_cells, or the overwrite epilogue of the streaming kernel): the kernel gets no
// counter pointers, and a table there must be -- the context's scratch when the caller wants no cells (or no cell tokens).
int counters_from_cells(scv_ctx* ctx, const AggCall& c, scv::AggArgs& a) {
    a.tie_hits = nullptr; a.token_sum = nullptr; a.truth_sum = nullptr;
    if (!a.cells || (c.tok() && c.tok_sum && !a.cell_tokens)) {
        const size_t cb = (size_t)a.ncells * sizeof(scv_cell);
        if (int rc = ensure_cells(ctx, cb + (size_t)a.ncells * sizeof(int64_t) + 256)) return rc;
        if (!a.cells) a.cells = static_cast<scv_cell*>(ctx->d_cells);
        if (c.tok() && !a.cell_tokens) a.cell_tokens = reinterpret_cast<int64_t*>(static_cast<char*>(ctx->d_cells) + ((cb + 255) / 256) * 256);
    }
    return SCV_OK;
}

int launch_reduce_cells(scv_ctx* ctx, const AggCall& c, const scv::AggArgs& a) {
    const dim3 grid((unsigned)plan::reduce_chunks(c.P, c.B, ctx->num_cus), (unsigned)(c.B < 65535 ? c.B : 65535));
    auto u64 = [](int64_t* p) { return reinterpret_cast<unsigned long long*>(p); };
    auto *th = u64(c.tie), *ts = u64(c.tok_sum), *tc = u64(c.truth_sum);
    // token reads only when token_sum is wanted: cell_tokens scratch exists exactly then
    if (c.tok() && c.tok_sum) hipLaunchKernelGGL((scv::scv_reduce_cells<true>), grid, dim3(256), 0, ctx->stream, a.cells, a.cell_tokens, c.P, c.B, th, ts, tc);
    else hipLaunchKernelGGL((scv::scv_reduce_cells<false>), grid, dim3(256), 0, ctx->stream, a.cells, a.cell_tokens, c.P, c.B, th, ts, tc);
    SCV_HIP(hipGetLastError());
    return SCV_OK;
}

// The event pair around the launches of one call (nothing without SCV_FLAG_TIMING): open() takes the pair, start() is queued right in front
// of the first launch -- behind the memset nodes and the host-side queries -- and stop() behind the last.
struct TimedSpan {
    EventPair* ev = nullptr;
    int open(scv_ctx* ctx) { return next_event_pair(ctx, &ev); }
    int start(scv_ctx* ctx) { if (ev) SCV_HIP(hipEventRecord(ev->a, ctx->stream)); return SCV_OK; }
    int stop(scv_ctx* ctx) { if (ev) SCV_HIP(hipEventRecord(ev->b, ctx->stream)); return SCV_OK; }
};

// Behind the hot kernel of a call: its launch error, the counters from the cell table if they were not computed in the launch, the closing event.
int finish(scv_ctx* ctx, const AggCall& c, const scv::AggArgs& a, bool use_reduce, TimedSpan& span) {
    SCV_HIP(hipGetLastError());
    if (use_reduce)
        if (int rc = launch_reduce_cells(ctx, c, a)) return rc;
    if (int rc = span.stop(ctx)) return rc;
    ctx->err_dirty = true;
    return SCV_OK;
}

// The kernel's LDS request, and how many of its workgroups the runtime says a CU holds (1 at least)
int resident_per_cu(KernelFn fn, int threads, size_t lds, int* per_cu) {
    SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SCV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, reinterpret_cast<const void*>(fn), threads, lds));
    if (*per_cu < 1) *per_cu = 1;
    return SCV_OK;
}

// ---- sorted cells: one lane per cell, the wave's 64 rows staged through LDS by LDS-DMA, sorted in registers (scvote_sort.hip.h).
// The reference's own range (N = 1 ... 128, o1.py:267,276).  Rows that are not all 16-byte aligned (N % 4 != 0, unaligned
// bases) take the linear-image form (dword reads).
// *fits = false, nothing queued: the launch does not fit the LDS (hundreds of budgets; plan::sort_fallback_kind says who takes the call)
// waves per workgroup of the sorted-cells launch of this call; 0: it does not fit the LDS
int sorted_cells_waves(const scv_ctx* ctx, const AggCall& c) {
    const int nv = plan::sort_nv(c.N);
    const RegKernel rk = pick_sort_kernel(nv, c.tok(), !c.rows_aligned());
    return plan::sort_waves(rk.waves, plan::sort_region_words(c.N, c.tok(), !c.rows_aligned()), plan::sort_tail_words(c.n_valid != nullptr, c.B, nv), ctx->lds_max);
}

int launch_sorted_cells(scv_ctx* ctx, const AggCall& c, scv::AggArgs& a, TimedSpan& span, bool* fits) {
    const int nv = plan::sort_nv(c.N);
    const RegKernel rk = pick_sort_kernel(nv, c.tok(), !c.rows_aligned());
    const int64_t region_words = plan::sort_region_words(c.N, c.tok(), !c.rows_aligned()), tail_words = plan::sort_tail_words(c.n_valid != nullptr, c.B, nv);
    const int W = sorted_cells_waves(ctx, c);
    if (!(*fits = W != 0)) return SCV_OK;
    a.wave_lds_words = (int32_t)region_words;
    const size_t lds = (size_t)(W * region_words + tail_words) * sizeof(uint32_t);
    SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rk.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t nsteps = (a.ncells + 63) / 64;
    // persistent: one workgroup per CU (or as many as the LDS lets be resident), 16 waves per CU at most
    int per_cu = ctx->lds_max / (int64_t)lds < 1 ? 1 : (int)(ctx->lds_max / (int64_t)lds);
    if (per_cu * W > 16) per_cu = 16 / W > 0 ? 16 / W : 1;
    // (few steps: smaller workgroups on more CUs, scvote_dispatch.h)
    const int Wl = scv::spread_waves(nsteps, W, ctx->num_cus, nv <= 16 ? 8 : 4);
    const size_t lds_l = (size_t)(Wl * region_words + tail_words) * sizeof(uint32_t);
    const int64_t grid = ctx->grid_override > 0 ? ctx->grid_override
                                                : plan::b_multiple_grid(std::min((nsteps + Wl - 1) / Wl, (int64_t)ctx->num_cus * per_cu), Wl * 64, c.B);
    ctx->stat_sort_cells += 1;
    if (int rc = span.start(ctx)) return rc;
    hipLaunchKernelGGL(rk.fn, dim3((unsigned)grid), dim3((unsigned)(Wl * 64)), lds_l, ctx->stream, a);
    return SCV_OK;
}

// ---- register-resident cells: workgroups of independent waves, 8 KiB of LDS each
// the register shape launch_reg_cells gives this call (plan::reg_shape; option "reg_shape" forces one)
plan::RegShape call_reg_shape(const scv_ctx* ctx, const AggCall& c) {
    const bool tok = c.tok(), vec = c.rows_aligned();
    const int64_t Nreg = vec ? c.N : c.N + 3;      // unaligned rows are read as their aligned supersets
    const int fv = ctx->reg_shape % 100;
    const bool have_g8 = ctx->reg_shape / 100 == 8 && (fv == 3 || fv == 4) && scv::pick_reg_g8(fv, tok, vec).fn != nullptr;
    return plan::reg_shape(Nreg, ctx->reg_shape, have_g8);
}

int launch_reg_cells(scv_ctx* ctx, const AggCall& c, scv::AggArgs& a, bool lds_counters, TimedSpan& span) {
    const bool tok = c.tok(), vec = c.rows_aligned();
    const plan::RegShape shape = call_reg_shape(ctx, c);
    const int64_t cpw = shape.h ? 1 : 64 / shape.g;
    const int64_t nbatches = (a.ncells + cpw - 1) / cpw;
    a.wave_lds_words = (int32_t)(scv::kRegWaveWords16 + plan::nv_cache_words(c.n_valid != nullptr, c.B));
    const RegKernel rk = shape.h ? pick_dense_kernel(shape.v, shape.h, tok, vec) : pick_reg_kernel(shape.g, shape.v, tok, vec);
    KernelFn fn = rk.fn;
    // workgroup = all the waves of the shape a CU holds (16 / 12 / 8: the kernel's launch bounds), fewer when the n_valid cache makes 16 regions overflow the LDS
    int WPG = rk.waves;
    while (WPG > 4 && (int64_t)WPG * a.wave_lds_words * 4 + 1024 > ctx->lds_max) WPG -= 4;
    size_t lds = (size_t)WPG * a.wave_lds_words * sizeof(uint32_t);
    // a surplus workgroup of the persistent grid would start only when another one has finished ALL its batches (measured 2x): ask the runtime
    int per_cu = 0;
    if (int rc = resident_per_cu(fn, WPG * 64, lds, &per_cu)) return rc;
    // Per-budget counters in the LDS the resident workgroups leave free (no occupancy lost): no scv_reduce_cells launch, no cell scratch
    if (lds_counters) {
        if (const int64_t tcl = plan::lds_tie_classes((ctx->lds_max / per_cu - (int64_t)lds) / 4 - 64, c.B, c.N)) {
            a.acc_classes = (int32_t)tcl;
            lds += plan::tie_classes_lds(c.B, tcl);
            SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            int again = 0;
            SCV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&again, reinterpret_cast<const void*>(fn), WPG * 64, lds));
            if (again >= 1 && again < per_cu) per_cu = again;   // (not expected: the region was sized from the spare LDS)
            ctx->stat_lds_counters += 1;
        }
    }
    const int64_t grid = plan::reg_grid(ctx->grid_override > 0 ? ctx->grid_override : (int64_t)ctx->num_cus * per_cu, nbatches, WPG, c.B);
    if (int rc = span.start(ctx)) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(WPG * 64), lds, ctx->stream, a);
    return SCV_OK;
}

// ---- cells of exactly 1, 2 or 4 votes (scvote_plan.h few_votes)
int launch_few_votes(scv_ctx* ctx, const AggCall& c, const scv::AggArgs& a, const plan::FewVotes& f, TimedSpan& span) {
    const bool tok = c.tok();
    const dim3 grid((unsigned)f.grid), threads(1024);
    ctx->stat_few_votes += 1;
    if (int rc = span.start(ctx)) return rc;
    KernelFn fn;
    size_t lds = (size_t)c.B * (c.N == 1 ? 2 : 4) * sizeof(unsigned long long);
    if (f.one) {
        if (c.N == 1) fn = tok ? (KernelFn)scv::scv_one_vote<true> : (KernelFn)scv::scv_one_vote<false>;
        else fn = tok ? (KernelFn)scv::scv_two_votes<true> : (KernelFn)scv::scv_two_votes<false>;
        ctx->stat_one_vote += 1;
    } else {
        lds = plan::lane_kernel_lds(c.B, (int)c.N);
#define SCV_FEW(NVV) (tok ? (KernelFn)scv::scv_few_votes<NVV, true> : (KernelFn)scv::scv_few_votes<NVV, false>)
        fn = c.N == 1 ? SCV_FEW(1) : (c.N == 2 ? SCV_FEW(2) : SCV_FEW(4));
#undef SCV_FEW
    }
    hipLaunchKernelGGL(fn, grid, threads, lds, ctx->stream, a);
    return SCV_OK;
}

// ---- tiny cells, one lane per cell; counters accumulated in LDS and flushed by the same launch
int launch_lane_cells(scv_ctx* ctx, const plan::Options& o, const AggCall& c, scv::AggArgs& a, TimedSpan& span) {
    const bool tok = c.tok();
    const int nv = plan::lane_nv(c.N);
    const size_t lds = plan::lane_kernel_lds(c.B, nv);
    a.wave_lds_words = c.rows_aligned() ? 1 : 0;   // "vec" flag
    const int64_t grid = ctx->grid_override > 0 ? ctx->grid_override : plan::lane_grid(o, a.ncells, nv, tok, c.B);
    if (int rc = span.start(ctx)) return rc;
#define SCV_LANE(NVV, TT, TOKK) hipLaunchKernelGGL((scv::scv_lane_cells<NVV, TT, TOKK>), dim3((unsigned)grid), dim3(TT), lds, ctx->stream, a)
    if (nv == 4) { if (tok) SCV_LANE(4, 1024, true); else SCV_LANE(4, 1024, false); }
    else if (nv == 8) { if (tok) SCV_LANE(8, 1024, true); else SCV_LANE(8, 1024, false); }
    else if (nv == 16) { if (tok) SCV_LANE(16, 512, true); else SCV_LANE(16, 1024, false); }
    else SCV_LANE(32, 512, false);                              // (with tokens: REG, scvote_plan.h cell_kind)
#undef SCV_LANE
    return SCV_OK;
}

// ---- the streaming kernel: whole cells or split-N, the counters by per-cell atomics, by scv_reduce_cells or by the overwrite epilogue,
// and the bootstrap of scv_aggregate_bootstrap_i32 behind a grid barrier of the same launch
int launch_stream(scv_ctx* ctx, const plan::Options& o, const AggCall& c, scv::AggArgs& a) {
    const bool tok = c.tok(), want_counters = c.want_counters();
    const int64_t ncells = a.ncells, N = c.N;
    const plan::StreamBand band = plan::stream_band(o, N, ncells);
    const size_t lds = band.lds;
    if ((int64_t)lds > ctx->lds_max) return fail(SCV_ERR_ARG, "LDS request %zu exceeds device limit %lld", lds, (long long)ctx->lds_max);
    const int copies = band.copies, threads = band.threads, unroll = band.unroll;
    const int64_t slots = (int64_t)ctx->num_cus * band.wg_per_cu;
    const plan::Split sp = plan::split(o, N, ncells, slots);
    const int64_t S = sp.S, nitems = ncells * S, grid = plan::stream_grid(nitems, slots, ctx->grid_override);
    // the single-launch epilogues exist for the geometries the library picks itself (scvote_dispatch.h)
    const bool have_xtra = pick_kernel(copies, threads, unroll, tok, true) != nullptr;
    // the form of the counters, decided once: overwritten by the launch's last workgroup | memset nodes in front + accumulated in the
    // launch | (memset nodes +) scv_reduce_cells behind it
    const bool few_cells = plan::overwrite_few_cells(o, want_counters, ncells, c.B);
    const bool overwrite_fused = few_cells && S == 1 && have_xtra;
    const bool use_reduce = !few_cells && plan::counters_by_reduce(o, want_counters, true, ncells, c.B, N);
    if (ctx->overwrite_counters && want_counters && !overwrite_fused)
        if (int rc = clear_counters(ctx, c.tie, c.tok_sum, c.truth_sum, c.B)) return rc;
    if (overwrite_fused) {
        a.overwrite = 1;
        a.tickets = static_cast<uint32_t*>(ctx->d_tickets);
        a.ow_tie = a.tie_hits; a.ow_tok = a.token_sum; a.ow_truth = a.truth_sum;      // (counters_from_cells takes them from the kernel's own)
        ctx->stat_overwrite_fused += 1;
    }
    if (use_reduce || overwrite_fused)
        if (int rc = counters_from_cells(ctx, c, a)) return rc;
    TimedSpan span;
    if (int rc = span.open(ctx)) return rc;
    if (S > 1) {
        a.segs = (int32_t)S; a.seg_len = sp.seg_len;
        a.sorted = 0;                                        // split items are numbered cell-major
        const size_t hist_bytes = (size_t)ncells * scv::kBins * sizeof(uint32_t);
        if (int rc = ensure_partial(ctx, hist_bytes + (size_t)ncells * sizeof(long long) + 256)) return rc;
        a.partial = static_cast<uint32_t*>(ctx->d_partial);
        a.partial_tok = reinterpret_cast<long long*>(static_cast<char*>(ctx->d_partial) + ((hist_bytes + 255) / 256) * 256);
        a.tickets = static_cast<uint32_t*>(ctx->d_tickets);
    }
    // bootstrap inside this launch (scv_aggregate_bootstrap_i32): whole cells only, code table + counters in the
    // histogram's LDS, and the whole grid resident at once (it meets at a grid barrier)
    if (ctx->boot_req && ctx->boot_path <= 1 && S == 1 && a.cells && have_xtra) {
        const scv_ctx::BootReq& rq = *ctx->boot_req;
        const size_t need_words = (((size_t)c.B * rq.M + 3) & ~(size_t)3) + ((size_t)ncells + 1) / 2;
        KernelFn fx = pick_kernel(copies, threads, unroll, tok, true);
        int per_cu = 0;
        SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fx), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        SCV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fx), threads, lds));
        if (need_words <= (size_t)scv::kBins * copies && grid <= (int64_t)per_cu * ctx->num_cus && c.P <= 0xFFFFFFFFll) {
            a.boot = 1;
            a.boot_r0 = rq.r0; a.boot_r1 = rq.r1; a.boot_M = rq.M; a.boot_seed = rq.seed;
            a.boot_spins = (uint32_t)(ctx->boot_spin_limit > 0 ? ctx->boot_spin_limit : 1);
            a.boot_out = reinterpret_cast<unsigned long long*>(rq.out);
            a.tickets = static_cast<uint32_t*>(ctx->d_tickets);
        }
    }
    if (plan::use_dispenser(o, nitems, grid, a.seg_len))
        a.dispenser = static_cast<uint32_t*>(ctx->d_tickets) + 3;
    const bool xtra = a.overwrite != 0 || a.boot != 0;
    KernelFn fn = pick_kernel(copies, threads, unroll, tok, xtra);
    if (!fn) return fail(SCV_ERR_ARG, "streaming geometry copies=%d threads=%d unroll=%d is not instantiated (scv_set_tuning lists the ones that are)", copies, threads, unroll);
    SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (int rc = span.start(ctx)) return rc;
    bool launched = false;
    if (a.boot) {
        // The workgroups meet at a grid barrier: ask the runtime for a COOPERATIVE launch, which only starts when the
        // whole grid can be resident at once whatever else (other streams, RCCL's kernels, another process) is on the
        // device.  Not available while the stream is being captured into a graph: there the ordinary launch is used and
        // the bounded spin + the repair in scv_sync cover a grid that turned out not to be co-resident.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        if (ctx->boot_path == 0 && cap == hipStreamCaptureStatusNone) {
            void* kargs[] = {const_cast<scv::AggArgs*>(&a)};
            const hipError_t ce = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(fn), dim3((unsigned)grid), dim3((unsigned)threads), kargs, (unsigned)lds, ctx->stream);
            if (ce == hipSuccess) { launched = true; ctx->stat_boot_cooperative += 1; }
            else {
                // refused (grid too large for a cooperative launch right now, or no support): two kernels instead
                (void)hipGetLastError();
                a.boot = 0; a.boot_out = nullptr;
                fn = pick_kernel(copies, threads, unroll, tok, a.overwrite != 0);
                SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            }
        }
        if (a.boot) {
            const scv_ctx::BootReq& rq = *ctx->boot_req;
            ctx->boot_req->fused = true;
            ctx->stat_boot_fused += 1;
            ctx->boot_last = scv_ctx::BootLast{a.cells, c.P, c.B, rq.r0, rq.r1, rq.M, rq.seed, rq.out, true};
        }
    }
    if (!launched) hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)threads), lds, ctx->stream, a);
    return finish(ctx, c, a, use_reduce, span);
}

// Dense cells [P, B, N], or -- pool_rows -- prefix budgets over one pool [P, N] through the CELL kernels (register-resident / one lane per
// cell): cell (p, b) counts the first n_valid[b] votes of row p.  Only launch_prefix asks for that, after plan::pool_rows_eligible().
// Accumulates into the per-budget counters.
int launch_cells(scv_ctx* ctx, const plan::Options& o, const AggCall& c, bool pool_rows) {
    if (c.ncells() == 0) return SCV_OK;
    scv::AggArgs a = agg_args(ctx, c);
    a.pool_rows = pool_rows ? 1 : 0; a.prefetch = 1;
    plan::Kind kind = plan::cell_kind(o, c.N, c.B, c.rows_aligned(), c.tok(), pool_rows);
    // 4-byte records (aggregate_common has checked the call form and N <= 127): only the kernels of plan::packed_ok write them.  Options can send
    // such cells elsewhere ("reg_n_max" below N: the streaming kernel; "reg_shape" 1041 .. 1048: the dense parts), where a 16-byte record per cell
    // would overrun the caller's 4-byte-per-cell table: refused here, with the kernel that would RUN known and nothing queued yet.
    const bool packed = (ctx->flags & SCV_FLAG_PACKED_CELLS) && c.cells && !pool_rows;
    if (packed) {
        plan::Kind runs = kind;
        if (runs == plan::SORT && sorted_cells_waves(ctx, c) == 0) runs = plan::sort_fallback_kind(o, c.N, c.B);
        if (!plan::packed_ok(runs, call_reg_shape(ctx, c)))
            return fail(SCV_ERR_ARG, "SCV_FLAG_PACKED_CELLS: options reg_n_max=%d sort_n_max=%d reg_shape=%d send cells of N=%lld votes to a kernel that writes "
                                     "16-byte records (the streaming kernel or a dense register shape); call without a cell table or change the options",
                        ctx->reg_n_max, ctx->sort_n_max, ctx->reg_shape, (long long)c.N);
    }
    a.packed_cells = packed ? 1 : 0;
    if (kind == plan::STREAM) return launch_stream(ctx, o, c, a);
    // the cell kernels count in their own LDS tables (scv_reduce_cells only when forced) and accumulate: overwrite = memset nodes in front
    const bool want_counters = c.want_counters();
    const bool use_reduce = plan::counters_by_reduce(o, want_counters, false, a.ncells, c.B, c.N);
    if (ctx->overwrite_counters && want_counters)
        if (int rc = clear_counters(ctx, c.tie, c.tok_sum, c.truth_sum, c.B)) return rc;
    if (use_reduce)
        if (int rc = counters_from_cells(ctx, c, a)) return rc;
    TimedSpan span;
    if (int rc = span.open(ctx)) return rc;
    int rc = SCV_OK; bool fits = true;
    if (kind == plan::SORT) rc = launch_sorted_cells(ctx, c, a, span, &fits);
    if (!fits) kind = plan::sort_fallback_kind(o, c.N, c.B);
    if (kind == plan::REG) rc = launch_reg_cells(ctx, c, a, want_counters && !use_reduce, span);
    else if (kind == plan::LANE) {
        const plan::FewVotes few = plan::few_votes(o, c.N, c.B, a.ncells, c.bases_aligned(), pool_rows, ctx->grid_override);
        rc = few.ok ? launch_few_votes(ctx, c, a, few, span) : launch_lane_cells(ctx, o, c, a, span);
    }
    return rc ? rc : finish(ctx, c, a, use_reduce, span);
}

int launch_aggregate(scv_ctx* ctx, const AggCall& c) { return launch_cells(ctx, plan_options(ctx), c, false); }

// What the forms of one prefix call hand to each other: scv_sort_prefix may be queued in front of the general kernel inside ONE event pair
// and behind ONE set of memset nodes.
struct PrefixState {
    TimedSpan span;
    bool counters_cleared = false;
    int skip_sortable = 0;          // = nv of the scv_sort_prefix queued in front (AggArgs::skip_sortable)
    bool done = false;              // scv_sort_prefix has the whole call (the list is known to be served)
    // overwrite semantics: memset nodes in front (no fused variant here); the pair opened and started unless a form in front has done it
    int begin(scv_ctx* ctx, const AggCall& c) {
        if (ctx->overwrite_counters && c.want_counters() && !counters_cleared)
            if (int rc = clear_counters(ctx, c.tie, c.tok_sum, c.truth_sum, c.B)) return rc;
        if (span.ev) return SCV_OK;
        if (int rc = span.open(ctx)) return rc;
        return span.start(ctx);
    }
};

// One pass per problem over its pool row, every budget a snapshot of the running mode statistics (scvote_prefix.hip.h).
int launch_prefix_pool(scv_ctx* ctx, const plan::Options& o, const AggCall& c, PrefixState& st) {
    scv::AggArgs a = agg_args(ctx, c);
    a.skip_sortable = st.skip_sortable; a.pool_rows = 1;
    const bool want_counters = c.want_counters();
    const int g = plan::prefix_pool_lanes(o, c.N, c.rows_aligned());
    const RegKernel rk = pick_prefix_pool_kernel(g, c.tok(), c.rows_aligned());
    a.wave_lds_words = (int32_t)(scv::prefix_pool_hist_words(g) + scv::kPrefixPoolLaneWords);
    const size_t fixed_words = 2 * (size_t)c.B + scv::kPrefixPoolFixedWords;
    int W = rk.waves;
    while (W > 1 && ((size_t)W * a.wave_lds_words + fixed_words + 64) * 4 > (size_t)ctx->lds_max) --W;
    size_t lds = ((size_t)W * a.wave_lds_words + fixed_words) * sizeof(uint32_t);
    const bool use_reduce = plan::counters_by_reduce(o, want_counters, false, a.ncells, c.B, c.N);   // forced (tests): counters from the cell table
    if (use_reduce)
        if (int rc = counters_from_cells(ctx, c, a)) return rc;
    // per-budget counters in the LDS the histograms leave free, flushed by the same launch
    if (want_counters && !use_reduce) {
        if (const int64_t tcl = plan::lds_tie_classes(((int64_t)ctx->lds_max - (int64_t)lds) / 4 - 64, c.B, c.N)) {
            a.acc_classes = (int32_t)tcl;
            lds += plan::tie_classes_lds(c.B, tcl);
            ctx->stat_lds_counters += 1;
        }
    }
    int per_cu = 0;
    if (int rc = resident_per_cu(rk.fn, W * 64, lds, &per_cu)) return rc;
    const int64_t nbatches = (c.P + (64 / g) - 1) / (64 / g);
    const int64_t grid = std::min<int64_t>(ctx->grid_override > 0 ? ctx->grid_override : (int64_t)ctx->num_cus * per_cu, (nbatches + W - 1) / W);
    if (int rc = st.begin(ctx, c)) return rc;
    hipLaunchKernelGGL(rk.fn, dim3((unsigned)grid), dim3((unsigned)(W * 64)), lds, ctx->stream, a);
    SCV_HIP(hipGetLastError());
    ctx->stat_prefix_pool += 1;
    return finish(ctx, c, a, use_reduce, st.span);
}

// Budgets that are powers of two (and the whole row) over pools of 17 .. 128 votes: every budget out of ONE sort per problem
// (scv_sort_prefix; 68 .. 128 votes and their token steps: scvote_plan.h sort_prefix_eligible).  *nv_queued: its nv once launched; the kernel leaves
// without side effects when some budget is not of that form (the caller then queues the general kernel behind it, a.skip_sortable = nv).
int launch_sort_prefix(scv_ctx* ctx, const AggCall& c, bool promised, int* nv_queued) {
    const int nv = plan::sort_prefix_nv(c.N);
    const bool tok = c.tok();
    const RegKernel rk = pick_sort_prefix_kernel(nv, tok);
    const int64_t region_words = plan::sort_prefix_region_words(c.N, nv), tail_words = scv::sort_prefix_tail_words(nv, c.B);
    const int W = plan::sort_prefix_waves(rk.waves, region_words, tail_words, ctx->lds_max);
    if (W == 0) return SCV_OK;
    scv::AggArgs a = agg_args(ctx, c);
    a.pool_rows = 1;
    if (!tok) { a.cell_tokens = nullptr; a.token_sum = nullptr; }
    a.budgets_promised = promised ? 1 : 0;     // the list is KNOWN to be of the served form (promised by the caller: option prefix_path = 5, or read by a HOST-mode call)
    a.wave_lds_words = (int32_t)region_words;
    const size_t lds = (size_t)(W * region_words + tail_words) * sizeof(uint32_t);
    int per_cu = 0;
    if (int rc = resident_per_cu(rk.fn, W * 64, lds, &per_cu)) return rc;
    const int64_t nsteps = (c.P + 63) / 64;
    // fewer steps than the chip has wave slots: every CU gets a workgroup before any CU gets a second wave per SIMD (a step is ~1400 VALU instructions
    // per wave; two waves of a SIMD in the same step take turns: 4.9 against 2.6 us for the sort of a one-step launch)
    const int Wl = scv::spread_waves(nsteps, W, ctx->num_cus);
    const size_t lds_l = (size_t)(Wl * region_words + tail_words) * sizeof(uint32_t);
    const int64_t grid = ctx->grid_override > 0 ? ctx->grid_override : std::min((nsteps + Wl - 1) / Wl, (int64_t)ctx->num_cus * per_cu);
    hipLaunchKernelGGL(rk.fn, dim3((unsigned)grid), dim3((unsigned)(Wl * 64)), lds_l, ctx->stream, a);
    SCV_HIP(hipGetLastError());
    ctx->stat_prefix_sort += 1;
    if (tok && nv == 128 && (c.cell_tokens || c.tok_sum)) ctx->stat_prefix_tokens += 1;   // (launches with the token steps of scv_sort_prefix2<true>)
    ctx->err_dirty = true;
    *nv_queued = nv;
    return SCV_OK;
}

// The sort-prefix attempt of a prefix call.  The budgets live in n_valid: a HOST-mode call reads them; a DEVICE-mode call queues
// scv_sort_prefix AND the general kernel -- each decides from n_valid, in its first microsecond, whether the launch is its own.
int try_sort_prefix(scv_ctx* ctx, const AggCall& c, PrefixState& st) {
    // prefix_path = 5: the caller PROMISES budgets of that form (a DEVICE-mode call then queues scv_sort_prefix alone; a list that breaks
    // the promise is an error, reported like a domain error at the next synchronisation)
    const bool promised = ctx->prefix_path == 5;
    bool known = promised, served = true;
    if (ctx->nv_host) {
        known = true;
        for (int32_t b = 0; b < c.B && served; ++b) served = plan::budget_served(ctx->nv_host[b], c.N);
    }
    if (!served && promised) return fail(SCV_ERR_ARG, "prefix_path = 5 promises budgets that are 0, a power of two <= %d, or >= N", (int)plan::sort_prefix_np(c.N));
    if (!served) return SCV_OK;
    if (int rc = st.span.open(ctx)) return rc;
    if (ctx->overwrite_counters && c.want_counters()) {
        if (int rc = clear_counters(ctx, c.tie, c.tok_sum, c.truth_sum, c.B)) return rc;
        st.counters_cleared = true;
    }
    if (int rc = st.span.start(ctx)) return rc;
    if (int rc = launch_sort_prefix(ctx, c, known, &st.skip_sortable)) return rc;
    st.done = st.skip_sortable && known;
    return st.done ? st.span.stop(ctx) : SCV_OK;
}

// pools of up to 64 samples: one lane per problem, every budget out of one pass (scv_lane_prefix); its counters come out of the same launch
int launch_prefix_lane(scv_ctx* ctx, const AggCall& c, scv::AggArgs& a, const plan::PrefixLane& lane) {
    const bool tok = c.tok();
    a.wave_lds_words = c.rows_aligned() ? 1 : 0;   // "vec" flag
    // Workgroup size.  N <= 32: 1024 threads, one workgroup per CU (the end-of-launch flush is one device atomic per
    // workgroup and counter, ~12 ns each on one address).  N = 64 needs 95-151 VGPRs: 256 threads, as many workgroups
    // as are resident (measured 61-64 us against 84-86 us with 768 / 1024 threads, which spill or leave a second, nearly
    // empty round).  Snapshots are staged in LDS (24 bytes x 64 x B per wave with tokens), in smaller workgroups if need be
    // (plan::prefix_lane picked the size).
    const int T = lane.threads;
#define SCV_LP2(NVV, TBB) (tok ? (KernelFn)scv::scv_lane_prefix<NVV, TBB, true> : (KernelFn)scv::scv_lane_prefix<NVV, TBB, false>)
    const KernelFn fn = lane.nv == 4 ? SCV_LP2(4, 1024) : (lane.nv == 8 ? SCV_LP2(8, 1024) : (lane.nv == 16 ? SCV_LP2(16, 1024) : (lane.nv == 32 ? SCV_LP2(32, 1024) : SCV_LP2(64, 256))));
#undef SCV_LP2
    int per_cu = 0;
    if (int rc = resident_per_cu(fn, T, lane.lds_total, &per_cu)) return rc;
    if (T == 1024) per_cu = 1;
    const int64_t grid = ctx->grid_override > 0 ? ctx->grid_override : std::min((c.P + T - 1) / T, (int64_t)ctx->num_cus * per_cu);
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)T), lane.lds_total, ctx->stream, a);
    ctx->stat_prefix_lane += 1;
    return SCV_OK;
}

// one pass over the pool, a snapshot of the LDS histogram at every boundary (scv_prefix_hist): pools longer than 4096 votes
int launch_prefix_hist(scv_ctx* ctx, const AggCall& c, const scv::AggArgs& a) {
    const bool tok = c.tok();
    // the band: histogram copies, threads, workgroups per CU; lds = the copies + cross-wave scratch + order and sorted n_valid
    const int copies = c.N < 32768 ? 8 : 16, threads = c.N < 32768 ? 256 : (c.N < 262144 ? 512 : 1024), wg_per_cu = 1024 / threads;
    const size_t lds = ((size_t)scv::kBins * copies + scv::kRedWords + 2 * (size_t)scv::kMaxSortedB) * sizeof(uint32_t);
    const int64_t grid = plan::stream_grid(c.P, (int64_t)ctx->num_cus * wg_per_cu, 0);
    KernelFn fn;
    if (threads == 256) fn = tok ? (KernelFn)scv::scv_prefix_hist<3, 256, 4, true> : (KernelFn)scv::scv_prefix_hist<3, 256, 4, false>;
    else if (threads == 512) fn = tok ? (KernelFn)scv::scv_prefix_hist<4, 512, 4, true> : (KernelFn)scv::scv_prefix_hist<4, 512, 4, false>;
    else fn = tok ? (KernelFn)scv::scv_prefix_hist<4, 1024, 4, true> : (KernelFn)scv::scv_prefix_hist<4, 1024, 4, false>;
    SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)threads), lds, ctx->stream, a);
    return SCV_OK;
}

// Prefix budgets over one pool [P, N] (scv_aggregate_prefix_i32).  Same outputs as launch_aggregate on the dense [P, B, N]
// expansion.  Option "prefix_path" forces one of the forms (parity tests).
int launch_prefix(scv_ctx* ctx, const AggCall& c) {
    if (c.ncells() == 0) return SCV_OK;
    const int64_t P = c.P, N = c.N; const int32_t B = c.B;
    const plan::Options o = plan_options(ctx);
    const plan::PrefixLane lane = plan::prefix_lane(o, B, N, c.tok());
    const bool rows_aligned = c.rows_aligned();
    PrefixState st;
    if (plan::sort_prefix_eligible(o, P, B, N, rows_aligned))
        if (int rc = try_sort_prefix(ctx, c, st); rc || st.done) return rc;
    const plan::PrefixForm form = plan::prefix_form(o, B, N, rows_aligned, lane.ok, st.skip_sortable != 0);
    if (form == plan::PREFIX_POOL) return launch_prefix_pool(ctx, o, c, st);
    if (form == plan::PREFIX_CELLS) {
        ctx->stat_prefix_cells += 1;
        return launch_cells(ctx, o, c, true);
    }
    scv::AggArgs a = agg_args(ctx, c);
    a.skip_sortable = st.skip_sortable;
    // (scv_lane_prefix: the counters come out of the same launch)
    const bool use_reduce = form == plan::PREFIX_HIST && plan::counters_by_reduce(o, c.want_counters(), true, a.ncells, B, N);
    if (use_reduce)
        if (int rc = counters_from_cells(ctx, c, a)) return rc;
    if (int rc = st.begin(ctx, c)) return rc;
    if (int rc = form == plan::PREFIX_LANE ? launch_prefix_lane(ctx, c, a, lane) : launch_prefix_hist(ctx, c, a)) return rc;
    return finish(ctx, c, a, use_reduce, st.span);
}

// Read and clear the device error word (stream must be idle).
int fetch_err(scv_ctx* ctx, uint32_t* out, bool force = false) {
    *out = 0;
    if (!ctx->err_dirty && !force) return SCV_OK;
    SCV_HIP(hipMemcpyAsync(out, ctx->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SCV_HIP(hipMemsetAsync(ctx->d_err, 0, sizeof(uint32_t), ctx->stream));
    SCV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->err_dirty = false;
    return SCV_OK;
}

int recover_fused_bootstrap(scv_ctx* ctx, uint32_t* w);

int check_err_word(scv_ctx* ctx, uint32_t w) {
    if (w & 4u) {
        // A workgroup of the fused vote + bootstrap launch gave up at the grid barrier (the grid was not co-resident:
        // only possible for the non-cooperative form, e.g. inside a captured graph).  The vote part is complete -- every
        // workgroup writes its cells and counters BEFORE it arrives at the barrier -- so the evaluation is repaired here:
        // barrier state reset, the whole bootstrap re-run as a separate launch over the same cell table, bit cleared.
        if (int rc = recover_fused_bootstrap(ctx, &w)) return rc;
    }
    if ((w & 1u) && !(ctx->flags & SCV_FLAG_CLAMP_TO_INVALID_BIN))
        return fail(SCV_ERR_DOMAIN, "a vote outside bins 0..1023 was seen; results are invalid");
    if (w & 2u) return fail(SCV_ERR_ARG, "bootstrap / resample: a hit had n_modes >= M (resample_wide, open domain: or >= SCV_TIE_CLASSES)");
    if (w & 16u) return fail(SCV_ERR_ARG, "token_budget / shortest: a token count was negative; results are invalid");
    if (w & 32u) return fail(SCV_ERR_ARG, "weighted: a weight was outside 0..%d; results are invalid", SCV_WEIGHT_MAX);
    if (w & 64u) return fail(SCV_ERR_ARG, "adaptive: a rule flag had a bit other than SCV_STOP_DECIDED; results are invalid");
    if (w & 128u) return fail(SCV_ERR_ARG, "iid: a draw budget was above SCV_IID_MAX_DRAWS = %d; nothing was computed", SCV_IID_MAX_DRAWS);
    if (w & 8u) return fail(SCV_ERR_ARG, "prefix_path = 5 promised budgets that are 0, a power of two or >= N: the list in n_valid is not; nothing was computed");
    return SCV_OK;
}

int recover_fused_bootstrap(scv_ctx* ctx, uint32_t* w) {
    SCV_HIP(hipMemsetAsync(ctx->d_tickets, 0, 4 * sizeof(uint32_t), ctx->stream));      // arrivals / generation: a clean barrier again
    if (!ctx->boot_last.valid)
        return fail(SCV_ERR_ARG, "fused bootstrap: grid barrier timed out and the request is not known any more (graph replay of an older capture?); use option boot_path = 2");
    const scv_ctx::BootLast q = ctx->boot_last;
    *w &= ~(4u | 2u);                            // bit 1 (value 2: class overflow) is re-derived by the re-run over the complete table
    if (int rc = scv_bootstrap(ctx, q.cells, q.P, q.B, q.r0, q.r1, q.seed, q.M, SCV_MEM_DEVICE, q.out)) return rc;
    uint32_t again = 0;
    if (int rc = fetch_err(ctx, &again, true)) return rc;        // synchronises the stream
    *w |= again & ~4u;
    ctx->stat_boot_recovered += 1;
    return SCV_OK;
}

int ensure_stage(scv_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->d_stage_bytes) return SCV_OK;
    if (ctx->d_stage) { SCV_HIP(hipFree(ctx->d_stage)); ctx->d_stage = nullptr; ctx->d_stage_bytes = 0; }
    SCV_HIP(hipMalloc(&ctx->d_stage, bytes));
    ctx->d_stage_bytes = bytes;
    return SCV_OK;
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The pinned block and the HBM block of the small HOST calls: "host_small_kb" KiB, or what the call needs if that is more.
int ensure_small_block(scv_ctx* ctx, size_t total) {
    if (total <= ctx->small_bytes) return SCV_OK;
    const size_t want = std::max((size_t)ctx->small_call_kb << 10, total);
    if (ctx->small_h) { SCV_HIP(hipHostFree(ctx->small_h)); ctx->small_h = nullptr; }
    if (ctx->small_d) { SCV_HIP(hipFree(ctx->small_d)); ctx->small_d = nullptr; }
    ctx->small_bytes = 0;
    SCV_HIP(hipHostMalloc(&ctx->small_h, want, hipHostMallocDefault));
    SCV_HIP(hipMalloc(&ctx->small_d, want));
    ctx->small_bytes = want;
    return SCV_OK;
}

const std::vector<double>& expected_table();     // scv_expected_majority_i32's binomials and Gauss-Legendre points (below)

}  // namespace

extern "C" {

const char* scv_last_error(void) { return g_err; }
#ifdef SCV_TEST_HOOKS
const char* scv_version(void) { return "scvote 0.2 (gfx950) +testhooks"; }
#else
const char* scv_version(void) { return "scvote 0.2 (gfx950)"; }
#endif

int scv_device_count(void) {
    return guarded([&]() -> int {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) return 0;
        return n;
    });
}

int scv_create(scv_ctx** out, int device, uint32_t flags) {
    return guarded([&]() -> int {
        if (!out) return fail(SCV_ERR_ARG, "scv_create: out is NULL");
        *out = nullptr;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SCV_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0) { SCV_HIP(hipGetDevice(&device)); }
        if (device >= n) return fail(SCV_ERR_ARG, "device %d out of range (%d visible)", device, n);
        scv_ctx* ctx = new (std::nothrow) scv_ctx();
        if (!ctx) return fail(SCV_ERR_ALLOC, "out of host memory");
        ctx->device = device;
        ctx->flags = flags;
        DeviceGuard guard_;                       // restores the caller's current device on every return path
        hipError_t e = guard_.enter(device) == SCV_OK ? hipSuccess : hipErrorInvalidDevice;
        hipDeviceProp_t prop;
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e == hipSuccess) { ctx->own_stream = true; e = hipMalloc((void**)&ctx->d_err, 256); }
        if (e == hipSuccess) e = hipMemset(ctx->d_err, 0, 256);
        if (e == hipSuccess) e = hipMalloc(&ctx->d_tickets, kTicketWords * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(ctx->d_tickets, 0, kTicketWords * sizeof(uint32_t));
        if (e == hipSuccess) { ctx->d_tickets_words = kTicketWords; e = hipDeviceSynchronize(); }
        const std::vector<double>& tab = expected_table();
        if (e == hipSuccess) { e = hipMalloc((void**)&ctx->d_expected_tab, tab.size() * sizeof(double)); }
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_expected_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            int code = fail(-(int)e, "scv_create: %s", hipGetErrorString(e));
            if (ctx->d_expected_tab) (void)hipFree(ctx->d_expected_tab);
            if (ctx->d_tickets) (void)hipFree(ctx->d_tickets);
            if (ctx->d_err) (void)hipFree(ctx->d_err);
            if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
            delete ctx;
            return code;
        }
        ctx->num_cus = prop.multiProcessorCount;
        ctx->lds_max = 160 * 1024;  // gfx950: a single workgroup may declare all 160 KiB
        ctx->clock_khz = prop.clockRate;
        ctx->hbm_bytes = (int64_t)prop.totalGlobalMem;
        *out = ctx;
        return SCV_OK;
    });
}

int scv_destroy(scv_ctx* ctx) {
    return guarded([&]() -> int {
        if (!ctx) return SCV_OK;
        DeviceGuard guard_;
        (void)guard_.enter(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (auto& ev : ctx->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
        if (ctx->pipe) { ctx->pipe->shutdown(); delete ctx->pipe; ctx->pipe = nullptr; }
        if (ctx->d_stage) (void)hipFree(ctx->d_stage);
        if (ctx->small_h) (void)hipHostFree(ctx->small_h);
        if (ctx->small_d) (void)hipFree(ctx->small_d);
        if (ctx->d_partial) (void)hipFree(ctx->d_partial);
        if (ctx->d_tickets) (void)hipFree(ctx->d_tickets);
        if (ctx->d_expected_tab) (void)hipFree(ctx->d_expected_tab);
        if (ctx->d_cells) (void)hipFree(ctx->d_cells);
        if (ctx->d_err) (void)hipFree(ctx->d_err);
        if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return SCV_OK;
    });
}

int scv_set_stream(scv_ctx* ctx, void* hip_stream) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        SCV_ENTER(ctx);
        // No synchronisation here (same contract as any set-stream call: ordering between the old and the
        // new stream is the caller's): a sync would be illegal while the new stream is being captured
        // into a hipGraph.  Only the ctx's own private stream is drained before it is destroyed.
        if (ctx->own_stream) {
            SCV_HIP(hipStreamSynchronize(ctx->stream));
            SCV_HIP(hipStreamDestroy(ctx->stream));
            ctx->own_stream = false;
        }
        ctx->stream = (hipStream_t)hip_stream;  // borrowed; NULL is the device's default stream
        return SCV_OK;
    });
}

int scv_sync(scv_ctx* ctx) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        SCV_ENTER(ctx);
        SCV_HIP(hipStreamSynchronize(ctx->stream));
        uint32_t w = 0;
        // always read the word (4 bytes): a hot path captured into a hipGraph is replayed without passing
        // through launch_aggregate, so the host-side dirty flag says nothing about replays
        if (int rc = fetch_err(ctx, &w, true)) return rc;
        return check_err_word(ctx, w);
    });
}

int scv_set_tuning(scv_ctx* ctx, int copies, int threads, int wg_per_cu, int unroll) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        if (copies < 0 && threads < 0 && wg_per_cu < 0 && unroll < 0) {      // all four negative: the library picks the geometry from the shape again
            ctx->copies = 16; ctx->threads = 1024; ctx->wg_per_cu = 1; ctx->unroll = 4;
            ctx->user_tuned = false;
            return SCV_OK;
        }
        const int c = copies > 0 ? copies : ctx->copies, t = threads > 0 ? threads : ctx->threads, u = unroll > 0 ? unroll : ctx->unroll;
        if (copies > 0 || threads > 0 || unroll > 0)
            if (!scv::pick_kernel(c, t, u, false, false))
                return fail(SCV_ERR_ARG, "streaming geometry copies=%d threads=%d unroll=%d is not instantiated: (copies, threads) in (4, 256) [unroll 2], "
                            "(8, 256) (8, 512) (16, 256) (16, 512) (16, 1024) [unroll 4]", c, t, u);
        ctx->copies = c; ctx->threads = t; ctx->unroll = u;
        if (wg_per_cu > 0) ctx->wg_per_cu = wg_per_cu;
        if (copies > 0 || threads > 0 || wg_per_cu > 0 || unroll > 0) ctx->user_tuned = true;   // explicit geometry wins over the auto choice
        return SCV_OK;
    });
}

int scv_set_option(scv_ctx* ctx, const char* key, int64_t value) {
    return guarded([&]() -> int {
        if (!ctx || !key) return fail(SCV_ERR_ARG, "NULL argument");
        if (!strcmp(key, "overwrite_counters")) ctx->overwrite_counters = value != 0;
        else if (!strcmp(key, "auto_geometry")) {
            // DEPRECATED alias (rounds 1-4 documented this key; round 5 replaced it by scv_set_tuning(ctx, -1, -1, -1, -1)): 1 = the library
            // picks the streaming geometry from the shape again; 0 = keep whatever scv_set_tuning set (and pin the current geometry)
            if (value) { ctx->copies = 16; ctx->threads = 1024; ctx->wg_per_cu = 1; ctx->unroll = 4; ctx->user_tuned = false; }
            else ctx->user_tuned = true;
        }
        else if (!strcmp(key, "path")) { if (value < 0 || value > 5) return fail(SCV_ERR_ARG, "path must be 0 .. 5"); ctx->path = (int)value; }
        else if (!strcmp(key, "sort_n_min")) { if (value < 1 || value > 65) return fail(SCV_ERR_ARG, "sort_n_min must be 1..65"); ctx->sort_n_min = (int)value; }
        else if (!strcmp(key, "sort_n_max")) { if (value < 0 || value > 64) return fail(SCV_ERR_ARG, "sort_n_max must be 0..64"); ctx->sort_n_max = (int)value; }
        else if (!strcmp(key, "reg_n_max")) { if (value < 0) return fail(SCV_ERR_ARG, "reg_n_max < 0"); ctx->reg_n_max = (int)(value > 8192 ? 8192 : value); }
        else if (!strcmp(key, "reg_shape")) { if (value < 0 || value > 9999) return fail(SCV_ERR_ARG, "reg_shape out of range"); ctx->reg_shape = (int)value; }
        else if (!strcmp(key, "fused_counters_max")) { if (value < 0) return fail(SCV_ERR_ARG, "fused_counters_max < 0"); ctx->fused_counters_max = (int)(value > (1 << 30) ? (1 << 30) : value); }
        else if (!strcmp(key, "grid")) { if (value < 0 || value > (1 << 20)) return fail(SCV_ERR_ARG, "grid out of range"); ctx->grid_override = (int)value; }
        else if (!strcmp(key, "segs")) { if (value < 0 || value > 4096) return fail(SCV_ERR_ARG, "segs out of range"); ctx->segs_override = (int)value; }
        else if (!strcmp(key, "prefix_path")) { if (value < 0 || value > 5) return fail(SCV_ERR_ARG, "prefix_path must be 0..5"); ctx->prefix_path = (int)value; }
        else if (!strcmp(key, "boot_path")) { if (value < 0 || value > 3) return fail(SCV_ERR_ARG, "boot_path must be 0..3"); ctx->boot_path = (int)value; }
        else if (!strcmp(key, "boot_spin_limit")) { if (value < 1 || value > (1 << 30)) return fail(SCV_ERR_ARG, "boot_spin_limit out of range"); ctx->boot_spin_limit = (int)value; }
        else if (!strcmp(key, "stage_mb")) { if (value < 1 || value > 65536) return fail(SCV_ERR_ARG, "stage_mb out of range"); ctx->stage_mb = (int)value; }
        else if (!strcmp(key, "host_small_kb")) { if (value < 0 || value > (1 << 20)) return fail(SCV_ERR_ARG, "host_small_kb out of range"); ctx->small_call_kb = (int)value; }
        else if (!strcmp(key, "copy_threads")) { if (value < 1 || value > 256) return fail(SCV_ERR_ARG, "copy_threads out of range"); ctx->copy_threads = (int)value; }
        else return fail(SCV_ERR_ARG, "unknown option '%s'", key);
        return SCV_OK;
    });
}

}  // extern "C" (reopened below)

namespace {

bool is_pinned_host(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}

int ensure_pipe(scv_ctx* ctx, size_t bounce_bytes, size_t dslot_bytes) {
    if (!ctx->pipe) {
        ctx->pipe = new (std::nothrow) HostPipe();
        if (!ctx->pipe) return fail(SCV_ERR_ALLOC, "out of host memory");
        SCV_HIP(hipStreamCreateWithFlags(&ctx->pipe->copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < HostPipe::kSlots; ++k) {
            SCV_HIP(hipEventCreateWithFlags(&ctx->pipe->landed[k], hipEventDisableTiming));
            SCV_HIP(hipEventCreateWithFlags(&ctx->pipe->consumed[k], hipEventDisableTiming));
        }
    }
    HostPipe* hp = ctx->pipe;
    int nthreads = ctx->copy_threads - 1;                      // the calling thread copies too
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0 && nthreads > hw - 1) nthreads = hw - 1;
    if (nthreads > 0) hp->start(nthreads, test_fault() == 1);
    if (bounce_bytes > hp->bounce_bytes) {
        for (int k = 0; k < HostPipe::kSlots; ++k) {
            if (hp->bounce[k]) { SCV_HIP(hipHostFree(hp->bounce[k])); hp->bounce[k] = nullptr; }
            SCV_HIP(hipHostMalloc(&hp->bounce[k], bounce_bytes, hipHostMallocDefault));
        }
        hp->bounce_bytes = bounce_bytes;
    }
    if (dslot_bytes > hp->dslot_bytes) {
        for (int k = 0; k < HostPipe::kSlots; ++k) {
            if (hp->dslot[k]) { SCV_HIP(hipFree(hp->dslot[k])); hp->dslot[k] = nullptr; }
            SCV_HIP(hipMalloc(&hp->dslot[k], dslot_bytes));
        }
        hp->dslot_bytes = dslot_bytes;
    }
    return SCV_OK;
}

using scv::add_copy_pieces;     // memcpy split over the pipe's worker threads (scvote_hostpool.h)

// HOST mode: the three-stage ingestion pipeline described at HostPipe.
int host_pipelined(scv_ctx* ctx, bool prefix, const int32_t* answers, const int32_t* tokens, const int32_t* n_valid,
                   const int32_t* truth, int64_t P, int32_t B, int64_t N, scv_cell* cells_out, int64_t* cell_tokens_out,
                   int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* truth_count_sum_out) {
    auto launch = prefix ? launch_prefix : launch_aggregate;
    const size_t row_bytes = (prefix ? (size_t)1 : (size_t)B) * (size_t)N * sizeof(int32_t);   // votes of one problem
    const size_t row_elems = row_bytes / sizeof(int32_t);
    const size_t per_problem = row_bytes * (tokens ? 2 : 1) + sizeof(int32_t);
    const size_t total = per_problem * (size_t)P;
    // chunk: at most stage_mb, and small enough that a call of a few tens of MB still overlaps copy and DMA
    size_t target = (size_t)(ctx->stage_mb > 0 ? ctx->stage_mb : 128) << 20;
    if (total / 8 < target) target = total / 8 > ((size_t)4 << 20) ? total / 8 : ((size_t)4 << 20);
    int64_t chunk = per_problem ? (int64_t)(target / per_problem) : P;
    if (chunk < 1) chunk = 1;
    if (chunk > P) chunk = P;
    // slot layout: inputs [answers | tokens | truth], outputs [cells | cell_tokens]
    size_t off = 0;
    const size_t o_ans = off; off = align_up(off + (size_t)chunk * row_bytes, 256);
    const size_t o_tok = off; off = align_up(off + (tokens ? (size_t)chunk * row_bytes : 0), 256);
    const size_t o_truth = off; off = align_up(off + (size_t)chunk * sizeof(int32_t), 256);
    const size_t in_bytes = off;
    const size_t o_cells = off; off = align_up(off + (size_t)chunk * B * sizeof(scv_cell), 256);
    const size_t o_ctok = off; off = align_up(off + (size_t)chunk * B * sizeof(int64_t), 256);
    const size_t slot_bytes = off > 0 ? off : 256;
    if (int rc = ensure_pipe(ctx, slot_bytes, slot_bytes)) return rc;
    HostPipe* hp = ctx->pipe;
    // per-call device block: n_valid + counters
    const size_t counters_bytes = ((size_t)B * SCV_TIE_CLASSES + 2 * (size_t)B) * sizeof(int64_t);
    const size_t o_nv = 0, o_cnt = align_up((size_t)B * sizeof(int32_t), 256);
    if (int rc = ensure_stage(ctx, o_cnt + align_up(counters_bytes, 256) + 256)) return rc;
    char* sbase = static_cast<char*>(ctx->d_stage);
    int64_t* d_tie = reinterpret_cast<int64_t*>(sbase + o_cnt);
    int64_t* d_tok = d_tie + (size_t)B * SCV_TIE_CLASSES;
    int64_t* d_ts = d_tok + B;
    hipStream_t s = ctx->stream, cs = hp->copy_stream;
    // the kernels report into the block's own error word for this call, as in host_small and stage_call (restored on every path): what a DEVICE-mode
    // call queued earlier left in the context's word stays there for scv_sync
    const size_t o_err = o_cnt + align_up(counters_bytes, 256);
    SCV_HIP(hipMemsetAsync(sbase + o_cnt, 0, o_err + sizeof(uint32_t) - o_cnt, s));
    struct ErrSwap { scv_ctx* c; uint32_t* keep; bool dirty; ~ErrSwap() { c->d_err = keep; c->err_dirty = dirty; } } swap{ctx, ctx->d_err, ctx->err_dirty};
    ctx->d_err = reinterpret_cast<uint32_t*>(sbase + o_err);
    if (n_valid && B > 0) SCV_HIP(hipMemcpyAsync(sbase + o_nv, n_valid, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // buffers the caller pinned are DMA'd in place; pageable ones go through the pinned bounce slots
    const bool pin_a = is_pinned_host(answers), pin_t = !tokens || is_pinned_host(tokens);
    const int parts = ctx->copy_threads > 0 ? ctx->copy_threads : 1;

    struct InFlight { int64_t p0 = 0, pc = 0; bool used = false; } slotinfo[HostPipe::kSlots];
    auto retire = [&](int k) -> int {                      // chunk in slot k is done: hand its cell table to the caller
        if (!slotinfo[k].used) return SCV_OK;
        SCV_HIP(hipEventSynchronize(hp->consumed[k]));
        const char* bb = static_cast<const char*>(hp->bounce[k]);
        const int64_t p0 = slotinfo[k].p0, pc = slotinfo[k].pc;
        if (cells_out && B > 0) memcpy(cells_out + (size_t)p0 * B, bb + o_cells, (size_t)pc * B * sizeof(scv_cell));
        if (cell_tokens_out && B > 0) memcpy(cell_tokens_out + (size_t)p0 * B, bb + o_ctok, (size_t)pc * B * sizeof(int64_t));
        slotinfo[k].used = false;
        return SCV_OK;
    };

    int64_t idx = 0;
    for (int64_t p0 = 0; p0 < P; p0 += chunk, ++idx) {
        const int k = (int)(idx % HostPipe::kSlots);
        const int64_t pc = (P - p0 < chunk) ? (P - p0) : chunk;
        if (int rc = retire(k)) return rc;                 // slot k (bounce + HBM) is free again
        char* bb = static_cast<char*>(hp->bounce[k]);
        char* db = static_cast<char*>(hp->dslot[k]);
        // stage 1: caller memory -> pinned bounce slot (worker threads); overlaps the DMA of the previous chunk
        std::vector<std::function<void()>> pieces;
        if (const int tf = test_fault(); tf == 2 || tf == 3) { if (tf == 2) throw std::bad_alloc(); throw std::runtime_error("test hook: SCV_TEST_FAULT=throw"); }
#ifdef SCV_TEST_HOOKS
        if (test_fault() == 4) {                               // (test builds only) unsynchronised increments from the copy workers
            static volatile long racy = 0;
            for (int r = 0; r < 8; ++r) pieces.emplace_back([] { for (int k = 0; k < 20000; ++k) racy = racy + 1; });
        }
#endif
        if (!pin_a) add_copy_pieces(pieces, bb + o_ans, answers + (size_t)p0 * row_elems, (size_t)pc * row_bytes, parts);
        if (tokens && !pin_t) add_copy_pieces(pieces, bb + o_tok, tokens + (size_t)p0 * row_elems, (size_t)pc * row_bytes, parts);
        memcpy(bb + o_truth, truth + p0, (size_t)pc * sizeof(int32_t));
        hp->run(std::move(pieces));
        // stage 2: DMA to the HBM slot on the copy stream
        const void* src_a = pin_a ? static_cast<const void*>(answers + (size_t)p0 * row_elems) : static_cast<const void*>(bb + o_ans);
        if (row_bytes) SCV_HIP(hipMemcpyAsync(db + o_ans, src_a, (size_t)pc * row_bytes, hipMemcpyHostToDevice, cs));
        if (tokens && row_bytes) {
            const void* src_t = pin_t ? static_cast<const void*>(tokens + (size_t)p0 * row_elems) : static_cast<const void*>(bb + o_tok);
            SCV_HIP(hipMemcpyAsync(db + o_tok, src_t, (size_t)pc * row_bytes, hipMemcpyHostToDevice, cs));
        }
        SCV_HIP(hipMemcpyAsync(db + o_truth, bb + o_truth, (size_t)pc * sizeof(int32_t), hipMemcpyHostToDevice, cs));
        SCV_HIP(hipEventRecord(hp->landed[k], cs));
        // stage 3: hot path on the compute stream, cell table back into the pinned slot
        SCV_HIP(hipStreamWaitEvent(s, hp->landed[k], 0));
        if (int rc = launch(ctx, AggCall{reinterpret_cast<const int32_t*>(db + o_ans),
                            tokens ? reinterpret_cast<const int32_t*>(db + o_tok) : nullptr,
                            n_valid ? reinterpret_cast<const int32_t*>(sbase + o_nv) : nullptr,
                            reinterpret_cast<const int32_t*>(db + o_truth), pc, B, N,
                            reinterpret_cast<scv_cell*>(db + o_cells), reinterpret_cast<int64_t*>(db + o_ctok), d_tie, d_tok, d_ts}))
            return rc;
        if (cells_out && B > 0) SCV_HIP(hipMemcpyAsync(bb + o_cells, db + o_cells, (size_t)pc * B * sizeof(scv_cell), hipMemcpyDeviceToHost, s));
        if (cell_tokens_out && B > 0) SCV_HIP(hipMemcpyAsync(bb + o_ctok, db + o_ctok, (size_t)pc * B * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        SCV_HIP(hipEventRecord(hp->consumed[k], s));
        // the copy stream may not overwrite this HBM slot before the kernel has consumed it (next use: chunk idx + 2,
        // whose retire(k) synchronises the host on consumed[k] before anything is enqueued)
        slotinfo[k].p0 = p0; slotinfo[k].pc = pc; slotinfo[k].used = true;
    }
    for (int k = 0; k < HostPipe::kSlots; ++k)
        if (int rc = retire(k)) return rc;
    if (B > 0) {
        if (tie_class_hits_out) SCV_HIP(hipMemcpyAsync(tie_class_hits_out, d_tie, (size_t)B * SCV_TIE_CLASSES * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (token_sum_out) SCV_HIP(hipMemcpyAsync(token_sum_out, d_tok, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (truth_count_sum_out) SCV_HIP(hipMemcpyAsync(truth_count_sum_out, d_ts, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    uint32_t w = 0;
    SCV_HIP(hipMemcpyAsync(&w, ctx->d_err, sizeof w, hipMemcpyDeviceToHost, s));
    SCV_HIP(hipStreamSynchronize(s));
    return check_err_word(ctx, w);
}

// HOST mode, small calls.  Every call the reference itself makes is tiny (P = 30 problems, N <= 128 samples, o1.py:277,302: a 15 KB
// tensor and a 10 us kernel), and the three-stage pipeline above -- built for GB-sized inputs -- cost it 0.25-0.4 ms of thread
// hand-offs, events and per-chunk copies.  Here the whole call is ONE pinned block and ONE HBM block owned by the ctx:
//     [ answers | tokens | truth | n_valid | counters = 0 | error word = 0 | cells | cell_tokens ]
//       `---------------- one H2D -------------------------------------'
//                                            `------------------- one D2H ------------------------'
// host memcpy in, one hipMemcpyAsync, the kernel, one hipMemcpyAsync back, one stream sync, host memcpy out.  No worker threads,
// no bounce slots, no per-call allocation; the kernels' error flag points into the block for the duration of the call, so the word
// arrives with the results and is zero again on the next call without a memset.
int host_small(scv_ctx* ctx, bool prefix, const int32_t* answers, const int32_t* tokens, const int32_t* n_valid,
               const int32_t* truth, int64_t P, int32_t B, int64_t N, scv_cell* cells_out, int64_t* cell_tokens_out,
               int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* truth_count_sum_out, bool* taken) {
    *taken = false;
    if (ctx->small_call_kb <= 0 || P <= 0 || B <= 0) return SCV_OK;
    const size_t votes_bytes = (size_t)P * (prefix ? (size_t)1 : (size_t)B) * (size_t)N * sizeof(int32_t);
    const size_t counters_bytes = ((size_t)B * SCV_TIE_CLASSES + 2 * (size_t)B) * sizeof(int64_t);
    size_t off = 0;
    const size_t o_ans = off; off = align_up(off + votes_bytes, 256);
    const size_t o_tok = off; off = align_up(off + (tokens ? votes_bytes : 0), 256);
    const size_t o_truth = off; off = align_up(off + (size_t)P * sizeof(int32_t), 256);
    const size_t o_nv = off; off = align_up(off + (size_t)B * sizeof(int32_t), 256);
    const size_t o_cnt = off; off = align_up(off + counters_bytes, 256);
    const size_t o_err = off; off += 256;
    const size_t h2d_bytes = off;
    const size_t o_cells = off; off = align_up(off + (size_t)P * B * sizeof(scv_cell), 256);
    const size_t o_ctok = off; off = align_up(off + (tokens ? (size_t)P * B * sizeof(int64_t) : 0), 256);
    const size_t total = off;
    if (total > (size_t)ctx->small_call_kb << 10) return SCV_OK;
    if (int rc = ensure_small_block(ctx, total)) return rc;
    *taken = true;
    ctx->stat_small_calls += 1;
    char* hb = static_cast<char*>(ctx->small_h);
    char* db = static_cast<char*>(ctx->small_d);
    if (votes_bytes) memcpy(hb + o_ans, answers, votes_bytes);
    if (tokens && votes_bytes) memcpy(hb + o_tok, tokens, votes_bytes);
    memcpy(hb + o_truth, truth, (size_t)P * sizeof(int32_t));
    if (n_valid) memcpy(hb + o_nv, n_valid, (size_t)B * sizeof(int32_t));
    memset(hb + o_cnt, 0, o_err + 256 - o_cnt);                       // counters + error word start at zero on the device too
    hipStream_t s = ctx->stream;
    SCV_HIP(hipMemcpyAsync(db, hb, h2d_bytes, hipMemcpyHostToDevice, s));
    int64_t* d_tie = reinterpret_cast<int64_t*>(db + o_cnt);
    int64_t* d_tok = d_tie + (size_t)B * SCV_TIE_CLASSES;
    int64_t* d_ts = d_tok + B;
    // the kernels report into the block's own error word for this call (restored on every path)
    struct ErrSwap { scv_ctx* c; uint32_t* keep; bool dirty; ~ErrSwap() { c->d_err = keep; c->err_dirty = dirty; } } swap{ctx, ctx->d_err, ctx->err_dirty};
    ctx->d_err = reinterpret_cast<uint32_t*>(db + o_err);
    auto launch = prefix ? launch_prefix : launch_aggregate;
    if (int rc = launch(ctx, AggCall{reinterpret_cast<const int32_t*>(db + o_ans), tokens ? reinterpret_cast<const int32_t*>(db + o_tok) : nullptr,
                        n_valid ? reinterpret_cast<const int32_t*>(db + o_nv) : nullptr, reinterpret_cast<const int32_t*>(db + o_truth), P, B, N,
                        reinterpret_cast<scv_cell*>(db + o_cells), tokens ? reinterpret_cast<int64_t*>(db + o_ctok) : nullptr, d_tie, d_tok, d_ts})) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    const bool want_cells = cells_out || cell_tokens_out;
    SCV_HIP(hipMemcpyAsync(hb + o_cnt, db + o_cnt, (want_cells ? total : o_cells) - o_cnt, hipMemcpyDeviceToHost, s));
    SCV_HIP(hipStreamSynchronize(s));
    uint32_t w = 0;
    memcpy(&w, hb + o_err, sizeof w);
    if (tie_class_hits_out) memcpy(tie_class_hits_out, hb + o_cnt, (size_t)B * SCV_TIE_CLASSES * sizeof(int64_t));
    if (token_sum_out) memcpy(token_sum_out, hb + o_cnt + (size_t)B * SCV_TIE_CLASSES * sizeof(int64_t), (size_t)B * sizeof(int64_t));
    if (truth_count_sum_out) memcpy(truth_count_sum_out, hb + o_cnt + ((size_t)B * SCV_TIE_CLASSES + B) * sizeof(int64_t), (size_t)B * sizeof(int64_t));
    if (cells_out) memcpy(cells_out, hb + o_cells, (size_t)P * B * sizeof(scv_cell));
    if (cell_tokens_out && tokens) memcpy(cell_tokens_out, hb + o_ctok, (size_t)P * B * sizeof(int64_t));
    return check_err_word(ctx, w);
}

// Shared body of scv_aggregate_i32 (dense: rows of B*N votes per problem) and
// scv_aggregate_prefix_i32 (prefix: one row of N votes per problem).
int aggregate_common(scv_ctx* ctx, bool prefix, const int32_t* answers, const int32_t* tokens, const int32_t* n_valid,
                     const int32_t* truth, int64_t P, int32_t B, int64_t N, int mem_kind, scv_cell* cells_out,
                     int64_t* cell_tokens_out, int64_t* tie_class_hits_out, int64_t* token_sum_out,
                     int64_t* truth_count_sum_out) {
    if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
    if (P < 0 || B < 0 || N < 0) return fail(SCV_ERR_ARG, "negative shape P=%lld B=%d N=%lld", (long long)P, B, (long long)N);
    if (N > 0x7fffffffll) return fail(SCV_ERR_ARG, "N=%lld exceeds 2^31-1 (cell counts are u32)", (long long)N);
    if (P > 0 && B > 0 && !truth) return fail(SCV_ERR_ARG, "truth is NULL");
    if (P > 0 && B > 0 && N > 0 && !answers) return fail(SCV_ERR_ARG, "answers is NULL");
    if (prefix && B > 0 && !n_valid) return fail(SCV_ERR_ARG, "prefix mode needs n_valid");
    if (prefix && B > scv::kMaxSortedB) return fail(SCV_ERR_ARG, "prefix mode supports at most %d budgets", scv::kMaxSortedB);
    if (mem_kind != SCV_MEM_HOST && mem_kind != SCV_MEM_DEVICE) return fail(SCV_ERR_ARG, "bad mem_kind %d", mem_kind);
    if ((ctx->flags & SCV_FLAG_PACKED_CELLS) && cells_out) {
        // 4-byte records: DEVICE-mode scv_aggregate_i32 over cells of up to 127 votes (every count fits 7 bits) on the kernels that serve such cells
        if (prefix || mem_kind != SCV_MEM_DEVICE || N > 127 || (ctx->path >= 1 && ctx->path <= 3) || ctx->fused_counters_max == 0 || ctx->boot_req)
            return fail(SCV_ERR_ARG, "SCV_FLAG_PACKED_CELLS: cells_out is uint32 [P, B] only for scv_aggregate_i32 on DEVICE memory with N <= 127 "
                                     "(auto dispatch; no prefix budgets, no bootstrap in the call); got prefix=%d mem_kind=%d N=%lld", (int)prefix, mem_kind, (long long)N);
    }
    if (mem_kind == SCV_MEM_DEVICE) {
        // The kernels store into the caller's arrays directly, with the widest store each output receives: 16 bytes for the two cell tables (whole
        // scv_cell records; four / two consecutive 4-byte records per lane of scv_one_vote / scv_two_votes; two consecutive cell_tokens per lane of
        // those kernels and of scv_sort_prefix), 8 bytes for the counters (64-bit atomics, the overwrite epilogue's 64-bit stores).  Nothing is queued
        // for a pointer below that.
        if ((((uintptr_t)cells_out | (uintptr_t)cell_tokens_out) & 15u) != 0)
            return fail(SCV_ERR_ARG, "DEVICE memory: cells_out and cell_tokens_out must be 16-byte aligned (got %p, %p)", (void*)cells_out, (void*)cell_tokens_out);
        if ((((uintptr_t)tie_class_hits_out | (uintptr_t)token_sum_out | (uintptr_t)truth_count_sum_out) & 7u) != 0)
            return fail(SCV_ERR_ARG, "DEVICE memory: tie_class_hits_out, token_sum_out and truth_count_sum_out must be 8-byte aligned (got %p, %p, %p)",
                        (void*)tie_class_hits_out, (void*)token_sum_out, (void*)truth_count_sum_out);
    }
    SCV_ENTER(ctx);
    auto launch = prefix ? launch_prefix : launch_aggregate;

    if (mem_kind == SCV_MEM_DEVICE)
        return launch(ctx, AggCall{answers, tokens, n_valid, truth, P, B, N, cells_out, cell_tokens_out, tie_class_hits_out, token_sum_out, truth_count_sum_out});

    // HOST mode accumulates its own zeroed counters over the chunks: the DEVICE-mode overwrite option must not apply
    struct Restore { scv_ctx* c; int v; ~Restore() { c->overwrite_counters = v; c->nv_host = nullptr; } } restore{ctx, ctx->overwrite_counters};
    ctx->overwrite_counters = 0;
    ctx->nv_host = prefix ? n_valid : nullptr;
    bool small = false;
    if (int rc = host_small(ctx, prefix, answers, tokens, n_valid, truth, P, B, N, cells_out, cell_tokens_out,
                            tie_class_hits_out, token_sum_out, truth_count_sum_out, &small)) return rc;
    if (small) return SCV_OK;
    ctx->stat_pipelined_calls += 1;
    return host_pipelined(ctx, prefix, answers, tokens, n_valid, truth, P, B, N, cells_out, cell_tokens_out,
                          tie_class_hits_out, token_sum_out, truth_count_sum_out);
}


// One launch of a lane-per-(problem, ordering) body of scv_resample_prefix (the shuffle, scvote_resample.hip.h; the token budgets,
// scvote_budget.hip.h; the weights, scvote_weighted.hip.h; the stopping rules, scvote_adaptive.hip.h; short-m@k, scvote_shortest.hip.h): a.P, a.R, a.N, a.B and the body's fields
// are set by the caller, a.np_max here.  Workgroups of 256 / 128 / 64 lanes:
// the one that keeps the most waves resident per CU (LDS: lds_words(lanes, rows a chunk touches) words -- the lanes' byte arrays, the
// problem rows, the per-budget tables), the larger on a tie (fewer tables to flush).  Persistent grid.  `what` prefixes the error message;
// stat_calls (NULL: the entry has no stat key) counts the launches.
template <class LdsWords>
int launch_lane_body(scv_ctx* ctx, scv::ResampleFn fn, scv::ResampleArgs& a, LdsWords lds_words, const char* what, int64_t* stat_calls) {
    const int64_t P = a.P, R = a.R;
    a.open_domain = (ctx->flags & SCV_FLAG_OPEN_DOMAIN) ? 1 : 0;        // every lane body encodes its rows by the context's rule
    SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->lds_max));
    int best_lanes = 0, best_np = 0, best_per_cu = 0;
    size_t best_lds = 0;
    for (int lanes = scv::kResampleMaxLanes; lanes >= 64; lanes >>= 1) {
        const int64_t np = std::min<int64_t>(P, (lanes - 1) / R + 2);
        const size_t lds = (size_t)lds_words(lanes, (int)np) * sizeof(uint32_t);
        if ((int64_t)lds > ctx->lds_max) continue;
        int per_cu = 0;
        SCV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), lanes, lds));
        if (per_cu < 1) continue;
        if (per_cu * lanes > best_per_cu * best_lanes) { best_lanes = lanes; best_np = (int)np; best_per_cu = per_cu; best_lds = lds; }
    }
    if (!best_lanes) return fail(SCV_ERR_ARG, "%s: N=%d B=%d does not fit the LDS of one workgroup", what, a.N, a.B);
    a.np_max = best_np;
    const int64_t nchunks = (P * R + best_lanes - 1) / best_lanes;
    int64_t grid = (int64_t)ctx->num_cus * best_per_cu;
    if (grid > nchunks) grid = nchunks;
    if (ctx->grid_override > 0) grid = ctx->grid_override;
    EventPair* ev = nullptr;
    if (int rc = next_event_pair(ctx, &ev)) return rc;
    if (ev) SCV_HIP(hipEventRecord(ev->a, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)best_lanes), best_lds, ctx->stream, a);
    SCV_HIP(hipGetLastError());
    if (ev) SCV_HIP(hipEventRecord(ev->b, ctx->stream));
    if (stat_calls) *stat_calls += 1;
    ctx->err_dirty = true;
    return SCV_OK;
}

// The fields of scv::ResampleArgs that every lane body reads (mode kResampleModeShuffle; what a body does not use is NULL): the launch wrappers
// below add their mode and their own fields.  The token sums are accumulated only with tokens.
scv::ResampleArgs lane_args(const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* truth, int64_t P, int32_t B, int64_t N,
                            int64_t p_offset, int order, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int64_t* tie, int64_t* tok_sum,
                            int64_t* truth_sum, int64_t* per_resample, uint32_t* err) {
    scv::ResampleArgs a{};
    a.pool = pool; a.tokens = tokens; a.n_valid = n_valid; a.truth = truth;
    a.P = P; a.p_offset = p_offset; a.seed = seed;
    a.N = (int32_t)N; a.B = B; a.R = (int32_t)((int64_t)r_end - r_begin); a.r_begin = r_begin; a.M = M;
    a.tie_hits = reinterpret_cast<unsigned long long*>(tie);
    a.token_sum = tokens ? reinterpret_cast<unsigned long long*>(tok_sum) : nullptr;
    a.truth_sum = reinterpret_cast<unsigned long long*>(truth_sum);
    a.per_resample = reinterpret_cast<unsigned long long*>(per_resample);
    a.err_flag = err;
    a.order = order == SCV_ORDER_SHUFFLED ? scv::kOrderShuffled : scv::kOrderPool;
    return a;
}

// scv_resample_prefix_i32 on device pointers: one launch of scv_resample_prefix<tok> (scvote_resample.hip.h), accumulating into the outputs.
int launch_resample(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* truth,
                    int64_t P, int32_t B, int64_t N, int64_t p_offset, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                    int64_t* tie, int64_t* tok_sum, int64_t* truth_sum, int64_t* per_resample, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    scv::ResampleArgs a = lane_args(pool, tokens, n_valid, truth, P, B, N, p_offset, SCV_ORDER_SHUFFLED, r_begin, r_end, seed, M, tie, tok_sum,
                                    truth_sum, per_resample, err);
    return launch_lane_body(ctx, pick_resample_kernel(tokens != nullptr), a,
                            [&](int lanes, int np) { return scv::resample_lds_words((int)N, B, lanes, np); }, "resample", &ctx->stat_resample_calls);
}

// scv_token_budget_prefix_i32 on device pointers: one launch of the token-budget body of scv_resample_prefix<true> (scvote_budget.hip.h),
// accumulating into the per-budget outputs and overwriting the cells.
int launch_token_budget(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int64_t* budgets, const int32_t* truth,
                        int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin, int32_t r_end, uint64_t seed,
                        int32_t M, int64_t* tie, int64_t* tok_sum, int64_t* vote_sum, int64_t* truth_sum, int64_t* per_resample,
                        scv_cell* cells, int64_t* cell_tokens, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    const bool shuffled = order == SCV_ORDER_SHUFFLED;
    scv::ResampleArgs a = lane_args(pool, tokens, nullptr, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M, tie, tok_sum, truth_sum,
                                    per_resample, err);
    a.mode = scv::kResampleModeTokenBudget;
    a.budgets = budgets;
    a.vote_sum = reinterpret_cast<unsigned long long*>(vote_sum);
    a.cells_out = cells; a.cell_tokens_out = cell_tokens;
    return launch_lane_body(ctx, pick_resample_kernel(true), a,
                            [&](int lanes, int np) { return scv::token_budget_lds_words((int)N, B, lanes, np, shuffled); }, "token_budget",
                            &ctx->stat_token_budget_calls);
}

// scv_weighted_prefix_i32 on device pointers: one launch of the weighted body of scv_resample_prefix<false> (scvote_weighted.hip.h),
// accumulating into the per-budget outputs and overwriting the cells.
int launch_weighted(scv_ctx* ctx, const int32_t* pool, const int32_t* weights, const int32_t* tokens, const int32_t* n_valid,
                    const int32_t* truth, int64_t P, int32_t B, int64_t N, int64_t p_offset, int rule, int order, int32_t r_begin,
                    int32_t r_end, uint64_t seed, int32_t M, int64_t* tie, int64_t* tok_sum, int64_t* per_resample, scv_cell* cells,
                    int64_t* cell_tokens, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    const bool shuffled = order == SCV_ORDER_SHUFFLED;
    const bool wlds = scv::weighted_rows_in_lds((int64_t)r_end - r_begin, shuffled);
    scv::ResampleArgs a = lane_args(pool, tokens, n_valid, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M, tie, tok_sum, nullptr,
                                    per_resample, err);
    a.mode = scv::kResampleModeWeighted;
    a.cells_out = cells; a.cell_tokens_out = cell_tokens;
    a.weights = weights; a.rule = rule; a.wlds = wlds ? 1 : 0;
    return launch_lane_body(ctx, pick_resample_kernel(false), a,
                            [&](int lanes, int np) { return scv::weighted_lds_words((int)N, B, lanes, np, shuffled, wlds); }, "weighted", nullptr);
}

// scv_adaptive_prefix_i32 on device pointers: one launch of the adaptive body of scv_resample_prefix<true> (scvote_adaptive.hip.h),
// accumulating into the per-rule outputs and overwriting the cells.
int launch_adaptive(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* cap, const int32_t* need,
                    const int32_t* rule_flags, const int32_t* truth, int64_t P, int32_t B, int64_t N, int64_t p_offset, int order,
                    int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int64_t* tie, int64_t* tok_sum, int64_t* vote_sum,
                    int64_t* truth_sum, int64_t* stop_hist, int64_t* per_resample, scv_cell* cells, int64_t* cell_tokens, int32_t* cell_votes,
                    uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    const bool shuffled = order == SCV_ORDER_SHUFFLED;
    scv::ResampleArgs a = lane_args(pool, tokens, nullptr, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M, tie, tok_sum, truth_sum,
                                    per_resample, err);
    a.mode = scv::kResampleModeAdaptive;
    a.vote_sum = reinterpret_cast<unsigned long long*>(vote_sum);
    a.cells_out = cells; a.cell_tokens_out = cell_tokens; a.cell_votes_out = cell_votes;
    a.cap = cap; a.need = need; a.rule_flags = rule_flags;
    a.stop_hist = reinterpret_cast<unsigned long long*>(stop_hist);
    return launch_lane_body(ctx, pick_resample_kernel(true), a,
                            [&](int lanes, int np) { return scv::adaptive_lds_words((int)N, B, lanes, np, shuffled); }, "adaptive", nullptr);
}

// scv_shortest_prefix_i32 on device pointers: one launch of the short-m@k body of scv_resample_prefix<true> (scvote_shortest.hip.h),
// accumulating into the per-budget outputs and overwriting the cells.
int launch_shortest(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* m_keep, const int32_t* truth,
                    int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                    int64_t* tie, int64_t* voted_sum, int64_t* spent_sum, int64_t* latency_sum, int64_t* truth_sum, int64_t* per_resample,
                    scv_cell* cells, int64_t* cell_tokens, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    const bool shuffled = order == SCV_ORDER_SHUFFLED;
    scv::ResampleArgs a = lane_args(pool, tokens, n_valid, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M, tie, voted_sum, truth_sum,
                                    per_resample, err);
    a.mode = scv::kResampleModeShortest;
    a.m_keep = m_keep;
    a.spent_sum = reinterpret_cast<unsigned long long*>(spent_sum);
    a.latency_sum = reinterpret_cast<unsigned long long*>(latency_sum);
    a.cells_out = cells; a.cell_tokens_out = cell_tokens;
    return launch_lane_body(ctx, pick_resample_kernel(true), a,
                            [&](int lanes, int np) { return scv::shortest_lds_words((int)N, B, lanes, np, shuffled); }, "shortest", nullptr);
}

// scv_iid_prefix_i32 on device pointers: one launch of the draws-with-replacement body of scv_resample_prefix<false> (scvote_iid.hip.h),
// accumulating into the outputs.
int launch_iid(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_draws, const int32_t* truth,
               int64_t P, int32_t B, int64_t N, int64_t p_offset, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
               int64_t* tie, int64_t* tok_sum, int64_t* truth_sum, int64_t* per_resample, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    scv::ResampleArgs a = lane_args(pool, tokens, n_draws, truth, P, B, N, p_offset, SCV_ORDER_SHUFFLED, r_begin, r_end, seed, M, tie, tok_sum,
                                    truth_sum, per_resample, err);
    a.mode = scv::kResampleModeIid;
    return launch_lane_body(ctx, pick_resample_kernel(false), a,
                            [&](int lanes, int np) { return scv::iid_lds_words((int)N, B, lanes, np); }, "iid", nullptr);
}

// The launch that the two wide entries share, behind the filling of `a`: one workgroup of wide_lanes(N) lanes per (problem, ordering) item with
// lds_bytes of LDS, a persistent grid of as many workgroups as stay resident, each with a contiguous run of items.  Not through
// launch_lane_body: no lanes to choose, no rows per chunk.  `what` names the entry in the refusal.
int launch_wide_items(scv_ctx* ctx, const scv::ResampleArgs& a, size_t lds_bytes, const char* what) {
    const scv::ResampleFn fn = pick_resample_kernel(false);
    const int lanes = scv::wide_lanes(a.N);
    if ((int64_t)lds_bytes > ctx->lds_max) return fail(SCV_ERR_ARG, "%s: N=%d B=%d does not fit the LDS of one workgroup", what, a.N, a.B);
    SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->lds_max));
    int per_cu = 0;
    SCV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), lanes, lds_bytes));
    if (per_cu < 1) per_cu = 1;
    const int64_t items = a.P * a.R;
    int64_t grid = (int64_t)ctx->num_cus * per_cu;
    if (grid > items) grid = items;
    if (ctx->grid_override > 0) grid = ctx->grid_override;
    EventPair* ev = nullptr;
    if (int rc = next_event_pair(ctx, &ev)) return rc;
    if (ev) SCV_HIP(hipEventRecord(ev->a, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)lanes), lds_bytes, ctx->stream, a);
    SCV_HIP(hipGetLastError());
    if (ev) SCV_HIP(hipEventRecord(ev->b, ctx->stream));
    ctx->err_dirty = true;
    return SCV_OK;
}

// scv_resample_wide_i32 on device pointers: one launch of the wide body of scv_resample_prefix<false> (scvote_wide.hip.h), accumulating into the
// outputs.  One workgroup per (problem, resample) item, its size and its LDS from N (wide_lanes, wide_lds_words: 51 KiB at N = 4096 with 13
// budgets, 61 KiB with 32 -- every N in range fits one workgroup), launched by launch_wide_items.  On a SCV_FLAG_OPEN_DOMAIN context the body
// encodes its rows by value and its histogram holds max(1024, N) 16-bit counts (55 KiB at N = 4096 with 13 budgets, 65 KiB with 32).
int launch_wide(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* truth,
                int64_t P, int32_t B, int64_t N, int64_t p_offset, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                int64_t* tie, int64_t* tok_sum, int64_t* truth_sum, int64_t* per_resample, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    scv::ResampleArgs a = lane_args(pool, tokens, n_valid, truth, P, B, N, p_offset, SCV_ORDER_SHUFFLED, r_begin, r_end, seed, M, tie, tok_sum,
                                    truth_sum, per_resample, err);
    a.mode = scv::kResampleModeWide;
    a.open_domain = (ctx->flags & SCV_FLAG_OPEN_DOMAIN) ? 1 : 0;
    return launch_wide_items(ctx, a, (size_t)scv::wide_lds_words((int)N, B, a.open_domain != 0) * sizeof(uint32_t), "resample_wide");
}

// scv_token_budget_wide_i32 on device pointers: one launch of the wide token-budget body of scv_resample_prefix<false>
// (scvote_wide_budget.hip.h), accumulating into the per-budget outputs and overwriting the cells.  The geometry of launch_wide: one workgroup per
// (problem, ordering) item, wide_lanes(N) lanes, a persistent grid of as many workgroups as stay resident; the LDS is wide_budget_lds_words
// (224 + 8 B bytes above the wide call's: 51 KiB at N = 4096 with 12 budgets, 55 KiB on a SCV_FLAG_OPEN_DOMAIN context).
int launch_wide_budget(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int64_t* budgets, const int32_t* truth,
                       int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin, int32_t r_end, uint64_t seed,
                       int32_t M, int64_t* tie, int64_t* tok_sum, int64_t* vote_sum, int64_t* truth_sum, int64_t* per_resample,
                       scv_cell* cells, int64_t* cell_tokens, uint32_t* err) {
    if (P == 0 || r_end == r_begin) return SCV_OK;
    scv::ResampleArgs a = lane_args(pool, tokens, nullptr, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M, tie, tok_sum, truth_sum,
                                    per_resample, err);
    a.mode = scv::kResampleModeWideBudget;
    a.open_domain = (ctx->flags & SCV_FLAG_OPEN_DOMAIN) ? 1 : 0;
    a.budgets = budgets;
    a.vote_sum = reinterpret_cast<unsigned long long*>(vote_sum);
    a.cells_out = cells; a.cell_tokens_out = cell_tokens;
    return launch_wide_items(ctx, a, (size_t)scv::wide_budget_lds_words((int)N, B, a.open_domain != 0) * sizeof(uint32_t), "token_budget_wide");
}

// The argument checks that scv_resample_prefix_i32, scv_token_budget_prefix_i32, scv_weighted_prefix_i32, scv_adaptive_prefix_i32,
// scv_shortest_prefix_i32 and scv_iid_prefix_i32 share, in
// the order the entries have always made them; `what` names the entry in every message.  An entry's own checks keep their places in that
// order: `early` runs behind the shape check (weighted: the rule), `own` behind the P * R bound (the pointers the entry requires).
// cells_given: the cell outputs of the entry as its message lists them when the caller passed one, NULL when it passed none.
// scv_resample_prefix_i32 has neither an order nor cells: it passes SCV_ORDER_SHUFFLED and NULL.  n_max: the largest pool of the entry (the lane
// bodies: kResampleMaxN; scv_resample_wide_i32 and scv_token_budget_wide_i32, which share the checks and the staging but not the lane layout:
// SCV_WIDE_MAX_N; the second also passes its order and its cells, as scv_token_budget_prefix_i32 does).
template <class Early, class Own>
int check_lane_call(const char* what, const scv_ctx* ctx, int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin,
                    int32_t r_end, const char* cells_given, bool per_resample, int32_t M, int mem_kind, Early early, Own own,
                    int n_max = scv::kResampleMaxN) {
    if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
    if (N < 1 || N > n_max || B < 1 || B > scv::kResampleMaxB || P < 0 || P > (1ll << 40) || p_offset < 0 || r_begin < 0 || r_end < r_begin)
        return fail(SCV_ERR_ARG, "%s: bad shape P=%lld B=%d N=%lld p_offset=%lld r=[%d,%d) (1 <= N <= %d, 1 <= B <= %d, 0 <= r_begin <= r_end)",
                    what, (long long)P, B, (long long)N, (long long)p_offset, r_begin, r_end, n_max, scv::kResampleMaxB);
    if (int rc = early()) return rc;
    if (order != SCV_ORDER_POOL && order != SCV_ORDER_SHUFFLED) return fail(SCV_ERR_ARG, "%s: bad order %d", what, order);
    if (order == SCV_ORDER_POOL && (r_begin != 0 || r_end != 1))
        return fail(SCV_ERR_ARG, "%s: SCV_ORDER_POOL is one draw: r_begin = 0, r_end = 1 (got [%d,%d))", what, r_begin, r_end);
    if (order == SCV_ORDER_SHUFFLED && cells_given) return fail(SCV_ERR_ARG, "%s: %s are written in SCV_ORDER_POOL only", what, cells_given);
    if (P > 0 && (int64_t)r_end - r_begin > (1ll << 62) / P) return fail(SCV_ERR_ARG, "%s: P * (r_end - r_begin) exceeds 2^62", what);
    if (int rc = own()) return rc;
    if (per_resample && M < 1) return fail(SCV_ERR_ARG, "%s: per_resample_out needs M >= 1 (got %d)", what, M);
    if (mem_kind != SCV_MEM_HOST && mem_kind != SCV_MEM_DEVICE) return fail(SCV_ERR_ARG, "bad mem_kind %d", mem_kind);
    return SCV_OK;
}
constexpr auto no_check = [] { return SCV_OK; };

// ---- HOST-mode staging of the lane-body entries and of scv_expected_majority_i32 ---------------------------------------------------------------
// A call is a table of regions, one per caller buffer.  ROWS regions hold `bytes` per problem and are staged a chunk of problems at a time: inputs
// go up in front of the chunk's launch, outputs (cells, cell tokens, cell votes, scores) come back behind it.  The inputs of the whole call (budgets,
// rules) go up ONCE; the outputs every chunk adds to (tie table, sums, stop histogram, per_resample: SUMS) are zeroed once on the device and come
// back once, at the end, with the error word.  A region whose caller pointer is NULL is absent: no room, no copy, a NULL device pointer.
struct Region {
    enum Kind { IN_ROWS, IN_ONCE, OUT_ROWS, OUT_SUMS } kind;
    void* host;
    size_t bytes;
    size_t off;                                             // where the region lies in the block (stage_layout)
    char* dev;                                              // ... and in device memory (stage_bind); NULL when absent
    bool rows() const { return kind == IN_ROWS || kind == OUT_ROWS; }
    template <class T> T* at() const { return reinterpret_cast<T*>(dev); }
};
Region rows_in(const void* host, size_t bytes_per_problem) { return {Region::IN_ROWS, const_cast<void*>(host), bytes_per_problem, 0, nullptr}; }
Region once_in(const void* host, size_t bytes) { return {Region::IN_ONCE, const_cast<void*>(host), bytes, 0, nullptr}; }
Region rows_out(void* host, size_t bytes_per_problem) { return {Region::OUT_ROWS, host, bytes_per_problem, 0, nullptr}; }
Region sums_out(void* host, size_t bytes) { return {Region::OUT_SUMS, host, bytes, 0, nullptr}; }

constexpr size_t kStageChunkBytes = (size_t)64 << 20;     // ROWS bytes of one chunk: bounds the device block whatever P is
constexpr size_t kWholeCall = (size_t)1 << 62;            // ... of a call that must stay one launch (scv_resample_prefix_i32)

// The block for chunks of `chunk` problems: [ every region but the sums, 256-byte aligned, in table order | the sums, back to back | error word ].
// Sets the regions' offsets; *o_sums, *o_err: where the sums and the error word begin.  Returns the size of the block.
size_t stage_layout(Region* rg, int n, int64_t chunk, size_t* o_sums, size_t* o_err) {
    size_t off = 0;
    for (Region* r = rg; r != rg + n; ++r) {
        if (r->kind == Region::OUT_SUMS) continue;
        r->off = off;
        off = align_up(off + (r->host ? r->bytes * (r->rows() ? (size_t)chunk : 1) : 0), 256);
    }
    *o_sums = off;
    for (Region* r = rg; r != rg + n; ++r) {
        if (r->kind != Region::OUT_SUMS) continue;
        r->off = off;
        off += r->host ? r->bytes : 0;
    }
    *o_err = align_up(off, 256);
    return *o_err + 256;
}

void stage_bind(Region* rg, int n, char* base) {
    for (Region* r = rg; r != rg + n; ++r) r->dev = r->host ? base + r->off : nullptr;
}

// A HOST call with nothing to vote on overwrites too: every output all zero.
int zero_outputs(const Region* rg, int n, int64_t P) {
    for (const Region* r = rg; r != rg + n; ++r)
        if (r->host && (r->kind == Region::OUT_ROWS || r->kind == Region::OUT_SUMS)) memset(r->host, 0, r->bytes * (r->rows() ? (size_t)P : 1));
    return SCV_OK;
}

// Runs a HOST call of P > 0 problems through the context's staging buffer, in chunks of as many problems as chunk_bytes of the present ROWS
// regions hold (at least one, at most P).  launch(np, p0, err) queues the kernel for problems [p0, p0 + np) on the regions' dev pointers; the
// kernels report into the block's own error word.  One stream sync between chunks (the next chunk overwrites the staged rows), one at the end.
template <class Launch>
int stage_call(scv_ctx* ctx, Region* rg, int n, int64_t P, size_t chunk_bytes, Launch launch) {
    size_t row_bytes = 0;
    for (const Region* r = rg; r != rg + n; ++r) if (r->host && r->rows()) row_bytes += r->bytes;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(chunk_bytes / row_bytes)));
    size_t o_sums = 0, o_err = 0;
    const size_t total = stage_layout(rg, n, chunk, &o_sums, &o_err);
    if (int rc = ensure_stage(ctx, total)) return rc;
    char* db = static_cast<char*>(ctx->d_stage);
    stage_bind(rg, n, db);
    uint32_t* d_err = reinterpret_cast<uint32_t*>(db + o_err);
    hipStream_t s = ctx->stream;
    for (const Region* r = rg; r != rg + n; ++r)
        if (r->host && r->kind == Region::IN_ONCE) SCV_HIP(hipMemcpyAsync(r->dev, r->host, r->bytes, hipMemcpyHostToDevice, s));
    SCV_HIP(hipMemsetAsync(db + o_sums, 0, total - o_sums, s));
    for (int64_t p0 = 0; p0 < P; p0 += chunk) {
        const int64_t np = std::min<int64_t>(chunk, P - p0);
        for (const Region* r = rg; r != rg + n; ++r)
            if (r->host && r->kind == Region::IN_ROWS)
                SCV_HIP(hipMemcpyAsync(r->dev, static_cast<const char*>(r->host) + (size_t)p0 * r->bytes, (size_t)np * r->bytes, hipMemcpyHostToDevice, s));
        if (int rc = launch(np, p0, d_err)) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        for (const Region* r = rg; r != rg + n; ++r)
            if (r->host && r->kind == Region::OUT_ROWS)
                SCV_HIP(hipMemcpyAsync(static_cast<char*>(r->host) + (size_t)p0 * r->bytes, r->dev, (size_t)np * r->bytes, hipMemcpyDeviceToHost, s));
        if (p0 + np < P) SCV_HIP(hipStreamSynchronize(s));
    }
    uint32_t w = 0;
    for (const Region* r = rg; r != rg + n; ++r)
        if (r->host && r->kind == Region::OUT_SUMS) SCV_HIP(hipMemcpyAsync(r->host, r->dev, r->bytes, hipMemcpyDeviceToHost, s));
    SCV_HIP(hipMemcpyAsync(&w, d_err, sizeof w, hipMemcpyDeviceToHost, s));
    SCV_HIP(hipStreamSynchronize(s));
    return check_err_word(ctx, w);
}

// scv_resample_prefix_i32 in HOST mode: ONE launch per call whatever its size.  Calls that fit "host_small_kb" (the reference's own sizes) go
// through the context's pinned block -- host memcpy in, one upload of the whole block, the kernel, one download of the sums and the error
// word, one stream sync, host memcpy out; larger ones through the staging buffer as a single chunk.
template <class Launch>
int resample_host(scv_ctx* ctx, Region* rg, int n, int64_t P, Launch launch) {
    size_t o_sums = 0, o_err = 0;
    const size_t total = stage_layout(rg, n, P, &o_sums, &o_err);
    if (ctx->small_call_kb <= 0 || total > ((size_t)ctx->small_call_kb << 10)) return stage_call(ctx, rg, n, P, kWholeCall, launch);
    if (int rc = ensure_small_block(ctx, total)) return rc;
    char* hb = static_cast<char*>(ctx->small_h);
    char* db = static_cast<char*>(ctx->small_d);
    stage_bind(rg, n, db);
    hipStream_t s = ctx->stream;
    for (const Region* r = rg; r != rg + n; ++r)
        if (r->host && (r->kind == Region::IN_ROWS || r->kind == Region::IN_ONCE)) memcpy(hb + r->off, r->host, r->bytes * (r->rows() ? (size_t)P : 1));
    memset(hb + o_sums, 0, total - o_sums);
    SCV_HIP(hipMemcpyAsync(db, hb, total, hipMemcpyHostToDevice, s));
    if (int rc = launch(P, 0, reinterpret_cast<uint32_t*>(db + o_err))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    SCV_HIP(hipMemcpyAsync(hb + o_sums, db + o_sums, total - o_sums, hipMemcpyDeviceToHost, s));
    SCV_HIP(hipStreamSynchronize(s));
    for (const Region* r = rg; r != rg + n; ++r)
        if (r->host && r->kind == Region::OUT_SUMS) memcpy(r->host, hb + r->off, r->bytes);
    uint32_t w = 0;
    memcpy(&w, hb + o_err, sizeof w);
    return check_err_word(ctx, w);
}

// The table (csrc/scvote_expected_table.h), built once per process.
const std::vector<double>& expected_table() {
    static const std::vector<double> tab = [] { std::vector<double> t; scv::build_expected_table(t); return t; }();
    return tab;
}


// scv_expected_majority_i32 on device pointers: the expected-mode body of scv_resample_prefix<false> (scvote_expected.hip.h), one workgroup
// of kExpectedLanes lanes per problem, persistent grid.  Overwrites score / hit rows [P, B].
int launch_expected(scv_ctx* ctx, const int32_t* pool, const int32_t* n_valid, const int32_t* truth, int64_t P, int32_t B, int64_t N,
                    double* score, double* hit, uint32_t* err) {
    if (P == 0) return SCV_OK;
    const scv::ResampleFn fn = pick_resample_kernel(false);
    const size_t lds = (size_t)scv::expected_lds_bytes(scv::kExpectedLanes);
    int per_cu = 0;
    SCV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), scv::kExpectedLanes, lds));
    if (per_cu < 1) per_cu = 1;
    scv::ResampleArgs a{};
    a.pool = pool; a.n_valid = n_valid; a.truth = truth;
    a.P = P; a.N = (int32_t)N; a.B = B;
    a.err_flag = err;
    a.mode = scv::kResampleModeExpected;
    a.tab = ctx->d_expected_tab;
    a.score_out = score; a.hit_out = hit;
    a.open_domain = (ctx->flags & SCV_FLAG_OPEN_DOMAIN) ? 1 : 0;        // (its own launch: not through launch_lane_body)
    int64_t grid = (int64_t)ctx->num_cus * per_cu;
    if (grid > P) grid = P;
    if (ctx->grid_override > 0) grid = ctx->grid_override;
    EventPair* ev = nullptr;
    if (int rc = next_event_pair(ctx, &ev)) return rc;
    if (ev) SCV_HIP(hipEventRecord(ev->a, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)scv::kExpectedLanes), lds, ctx->stream, a);
    SCV_HIP(hipGetLastError());
    if (ev) SCV_HIP(hipEventRecord(ev->b, ctx->stream));
    ctx->stat_expected_calls += 1;
    ctx->err_dirty = true;
    return SCV_OK;
}

}  // namespace

extern "C" {

int scv_aggregate_i32(scv_ctx* ctx, const int32_t* answers, const int32_t* tokens, const int32_t* n_valid,
                      const int32_t* truth, int64_t P, int32_t B, int64_t N, int mem_kind, scv_cell* cells_out,
                      int64_t* cell_tokens_out, int64_t* tie_class_hits_out, int64_t* token_sum_out,
                      int64_t* truth_count_sum_out) {
    return guarded([&]() -> int {
        return aggregate_common(ctx, false, answers, tokens, n_valid, truth, P, B, N, mem_kind, cells_out, cell_tokens_out,
                                tie_class_hits_out, token_sum_out, truth_count_sum_out);
    });
}

int scv_aggregate_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid,
                             const int32_t* truth, int64_t P, int32_t B, int64_t N, int mem_kind, scv_cell* cells_out,
                             int64_t* cell_tokens_out, int64_t* tie_class_hits_out, int64_t* token_sum_out,
                             int64_t* truth_count_sum_out) {
    return guarded([&]() -> int {
        return aggregate_common(ctx, true, pool, tokens, n_valid, truth, P, B, N, mem_kind, cells_out, cell_tokens_out,
                                tie_class_hits_out, token_sum_out, truth_count_sum_out);
    });
}

int scv_bootstrap(scv_ctx* ctx, const scv_cell* cells, int64_t P, int32_t B, int32_t r_begin, int32_t r_end,
                  uint64_t seed, int32_t M, int mem_kind, int64_t* counts_out) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        if (!cells || !counts_out) return fail(SCV_ERR_ARG, "bootstrap: NULL pointer");
        if (P <= 0 || P > 0xFFFFFFFFll || B <= 0 || M <= 0 || r_end < r_begin || r_begin < 0)
            return fail(SCV_ERR_ARG, "bootstrap: bad shape P=%lld B=%d M=%d r=[%d,%d)", (long long)P, B, M, r_begin, r_end);
        const size_t lds = (size_t)B * M * sizeof(uint32_t);
        if (lds > 64 * 1024) return fail(SCV_ERR_ARG, "bootstrap: B*M=%lld counters exceed 64 KiB of LDS", (long long)B * M);
        if (mem_kind != SCV_MEM_HOST && mem_kind != SCV_MEM_DEVICE) return fail(SCV_ERR_ARG, "bad mem_kind %d", mem_kind);
        SCV_ENTER(ctx);
        const int32_t R = r_end - r_begin;
        if (R == 0) return SCV_OK;
        hipStream_t s = ctx->stream;
        const size_t out_bytes = (size_t)R * B * M * sizeof(int64_t);
        // LDS-resident kernel when the 2-byte code table + counters fit (P * B up to ~70 k cells); otherwise the
        // global-gather kernel.  "boot_path" = 3 forces the latter (parity tests).
        const size_t lds_fast = (((size_t)B * M + 3) & ~(size_t)3) * sizeof(uint32_t) + (((size_t)P * B + 7) & ~(size_t)7) * sizeof(uint16_t);
        const bool fast = ctx->boot_path != 3 && lds_fast <= (size_t)144 * 1024;
        auto launch_boot = [&](const scv_cell* d_cells, unsigned long long* d_out, uint32_t* d_err) -> int {
            if (fast) {
                int64_t grid = (int64_t)ctx->num_cus;                          // one 1024-thread workgroup per CU, R / grid resamples each
                if (grid > R) grid = R;
                SCV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(scv::scv_bootstrap_lds_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fast));
                hipLaunchKernelGGL(scv::scv_bootstrap_lds_k, dim3((unsigned)grid), dim3(1024), lds_fast, s, d_cells, P, B, r_begin, r_end, seed, M, d_out, d_err);
            } else {
                hipLaunchKernelGGL(scv::scv_bootstrap_k, dim3((unsigned)R), dim3(256), lds, s, d_cells, P, B, r_begin, seed, M, d_out, d_err);
            }
            SCV_HIP(hipGetLastError());
            return SCV_OK;
        };
        if (mem_kind == SCV_MEM_DEVICE) {
            if (int rc = launch_boot(cells, reinterpret_cast<unsigned long long*>(counts_out), ctx->d_err)) return rc;
            ctx->err_dirty = true;
            return SCV_OK;
        }
        const size_t cells_bytes = (size_t)P * B * sizeof(scv_cell);
        const size_t o_out = align_up(cells_bytes, 256);
        // the kernel reports into the block's own error word for this call, as in host_small, stage_call and host_pipelined: what a
        // DEVICE-mode call queued earlier left in the context's word stays there, with err_dirty, for scv_sync
        const size_t o_err = align_up(o_out + out_bytes, 256);
        if (int rc = ensure_stage(ctx, o_err + 256)) return rc;
        char* base = static_cast<char*>(ctx->d_stage);
        uint32_t* d_err = reinterpret_cast<uint32_t*>(base + o_err);
        SCV_HIP(hipMemsetAsync(d_err, 0, sizeof(uint32_t), s));
        SCV_HIP(hipMemcpyAsync(base, cells, cells_bytes, hipMemcpyHostToDevice, s));
        if (int rc = launch_boot(reinterpret_cast<const scv_cell*>(base), reinterpret_cast<unsigned long long*>(base + o_out), d_err)) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        uint32_t w = 0;
        SCV_HIP(hipMemcpyAsync(counts_out, base + o_out, out_bytes, hipMemcpyDeviceToHost, s));
        SCV_HIP(hipMemcpyAsync(&w, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SCV_HIP(hipStreamSynchronize(s));
        return check_err_word(ctx, w);
    });
}

int scv_aggregate_bootstrap_i32(scv_ctx* ctx, const int32_t* answers, const int32_t* tokens, const int32_t* n_valid,
                                const int32_t* truth, int64_t P, int32_t B, int64_t N, scv_cell* cells_out,
                                int64_t* cell_tokens_out, int64_t* tie_class_hits_out, int64_t* token_sum_out,
                                int64_t* truth_count_sum_out, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                                int64_t* counts_out) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        if (!cells_out || !counts_out) return fail(SCV_ERR_ARG, "aggregate_bootstrap: cells_out and counts_out are required");
        if (ctx->flags & SCV_FLAG_PACKED_CELLS) return fail(SCV_ERR_ARG, "SCV_FLAG_PACKED_CELLS: vote + bootstrap in one call reads 16-byte records (use a ctx without the flag)");
        if (P <= 0 || P > 0xFFFFFFFFll || B <= 0 || M <= 0 || r_end < r_begin || r_begin < 0)
            return fail(SCV_ERR_ARG, "aggregate_bootstrap: bad shape P=%lld B=%d M=%d r=[%d,%d)", (long long)P, B, M, r_begin, r_end);
        if ((size_t)B * M * sizeof(uint32_t) > 64 * 1024) return fail(SCV_ERR_ARG, "bootstrap: B*M=%lld counters exceed 64 KiB of LDS", (long long)B * M);
        scv_ctx::BootReq rq{r_begin, r_end, M, seed, counts_out, false};
        if (r_end > r_begin) ctx->boot_req = &rq;
        const int rc = scv_aggregate_i32(ctx, answers, tokens, n_valid, truth, P, B, N, SCV_MEM_DEVICE, cells_out, cell_tokens_out,
                                         tie_class_hits_out, token_sum_out, truth_count_sum_out);
        ctx->boot_req = nullptr;
        if (rc != SCV_OK || rq.fused || r_end == r_begin) return rc;
        // shape or occupancy did not allow the fused form: the bootstrap is queued behind the vote on the same stream
        ctx->stat_boot_separate += 1;
        return scv_bootstrap(ctx, cells_out, P, B, r_begin, r_end, seed, M, SCV_MEM_DEVICE, counts_out);
    });
}

int scv_resample_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* truth,
                            int64_t P, int32_t B, int64_t N, int64_t p_offset, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                            int mem_kind, int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* truth_count_sum_out,
                            int64_t* per_resample_out) {
    return guarded([&]() -> int {
        if (int rc = check_lane_call("resample", ctx, P, B, N, p_offset, SCV_ORDER_SHUFFLED, r_begin, r_end, nullptr, per_resample_out, M, mem_kind, no_check, [&] {
                if (!n_valid || !tie_class_hits_out) return fail(SCV_ERR_ARG, "resample: n_valid and tie_class_hits_out are required");
                if (P > 0 && (!pool || !truth)) return fail(SCV_ERR_ARG, "resample: pool and truth are required");
                if (token_sum_out && !tokens) return fail(SCV_ERR_ARG, "resample: token_sum_out needs tokens");
                return SCV_OK;
            })) return rc;
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_resample(ctx, pool, tokens, n_valid, truth, P, B, N, p_offset, r_begin, r_end, seed, M, tie_class_hits_out,
                                   token_sum_out, truth_count_sum_out, per_resample_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t);
        enum { POOL, TOK, TRUTH, NV, TIE, TSUM, TCS, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(n_valid, (size_t)B * sizeof(int32_t)),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums), sums_out(truth_count_sum_out, sums),
                       sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing drawn, all zero
        return resample_host(ctx, rg, PER + 1, P, [&](int64_t np, int64_t p0, uint32_t* err) {
            return launch_resample(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[NV].at<const int32_t>(),
                                   rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, r_begin, r_end, seed, M, rg[TIE].at<int64_t>(),
                                   rg[TSUM].at<int64_t>(), rg[TCS].at<int64_t>(), rg[PER].at<int64_t>(), err);
        });
    });
}

int scv_token_budget_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int64_t* token_budget, const int32_t* truth,
                                int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin, int32_t r_end, uint64_t seed,
                                int32_t M, int mem_kind, int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* vote_count_sum_out,
                                int64_t* truth_count_sum_out, int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out) {
    return guarded([&]() -> int {
        const char* cells_given = (cells_out || cell_tokens_out) ? "cells_out / cell_tokens_out" : nullptr;
        if (int rc = check_lane_call("token_budget", ctx, P, B, N, p_offset, order, r_begin, r_end, cells_given, per_resample_out, M, mem_kind, no_check, [&] {
                if (!token_budget || !tie_class_hits_out) return fail(SCV_ERR_ARG, "token_budget: token_budget and tie_class_hits_out are required");
                if (P > 0 && (!pool || !tokens || !truth)) return fail(SCV_ERR_ARG, "token_budget: pool, tokens and truth are required");
                return SCV_OK;
            })) return rc;
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_token_budget(ctx, pool, tokens, token_budget, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M,
                                       tie_class_hits_out, token_sum_out, vote_count_sum_out, truth_count_sum_out, per_resample_out, cells_out,
                                       cell_tokens_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t);
        enum { POOL, TOK, TRUTH, BUD, CELLS, CTOK, TIE, TSUM, VSUM, TCS, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(token_budget, (size_t)B * sizeof(int64_t)),
                       rows_out(cells_out, (size_t)B * sizeof(scv_cell)), rows_out(cell_tokens_out, sums),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums), sums_out(vote_count_sum_out, sums),
                       sums_out(truth_count_sum_out, sums), sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing voted, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {
            return launch_token_budget(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[BUD].at<const int64_t>(),
                                       rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, order, r_begin, r_end, seed, M, rg[TIE].at<int64_t>(),
                                       rg[TSUM].at<int64_t>(), rg[VSUM].at<int64_t>(), rg[TCS].at<int64_t>(), rg[PER].at<int64_t>(),
                                       rg[CELLS].at<scv_cell>(), rg[CTOK].at<int64_t>(), err);
        });
    });
}

int scv_weighted_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* weights, const int32_t* tokens, const int32_t* n_valid,
                            const int32_t* truth, int64_t P, int32_t B, int64_t N, int64_t p_offset, int rule, int order, int32_t r_begin,
                            int32_t r_end, uint64_t seed, int32_t M, int mem_kind, int64_t* tie_class_hits_out, int64_t* token_sum_out,
                            int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out) {
    return guarded([&]() -> int {
        const char* cells_given = (cells_out || cell_tokens_out) ? "cells_out / cell_tokens_out" : nullptr;
        if (int rc = check_lane_call("weighted", ctx, P, B, N, p_offset, order, r_begin, r_end, cells_given, per_resample_out, M, mem_kind,
            [&] { return rule != SCV_RULE_WEIGHT_SUM && rule != SCV_RULE_BEST_OF ? fail(SCV_ERR_ARG, "weighted: bad rule %d", rule) : SCV_OK; },
            [&] {
                if (!n_valid || !tie_class_hits_out) return fail(SCV_ERR_ARG, "weighted: n_valid and tie_class_hits_out are required");
                if (!weights) return fail(SCV_ERR_ARG, "weighted: weights are required");
                if (P > 0 && (!pool || !truth)) return fail(SCV_ERR_ARG, "weighted: pool and truth are required");
                if ((token_sum_out || cell_tokens_out) && !tokens) return fail(SCV_ERR_ARG, "weighted: token_sum_out / cell_tokens_out need tokens");
                return SCV_OK;
            })) return rc;
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_weighted(ctx, pool, weights, tokens, n_valid, truth, P, B, N, p_offset, rule, order, r_begin, r_end, seed, M,
                                   tie_class_hits_out, token_sum_out, per_resample_out, cells_out, cell_tokens_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t);
        enum { POOL, WEIGHTS, TOK, TRUTH, NV, CELLS, CTOK, TIE, TSUM, PER };
        Region rg[] = {rows_in(pool, row), rows_in(weights, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)),
                       once_in(n_valid, (size_t)B * sizeof(int32_t)), rows_out(cells_out, (size_t)B * sizeof(scv_cell)), rows_out(cell_tokens_out, sums),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums),
                       sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing voted, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {
            return launch_weighted(ctx, rg[POOL].at<const int32_t>(), rg[WEIGHTS].at<const int32_t>(), rg[TOK].at<const int32_t>(),
                                   rg[NV].at<const int32_t>(), rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, rule, order, r_begin, r_end,
                                   seed, M, rg[TIE].at<int64_t>(), rg[TSUM].at<int64_t>(), rg[PER].at<int64_t>(), rg[CELLS].at<scv_cell>(),
                                   rg[CTOK].at<int64_t>(), err);
        });
    });
}

int scv_adaptive_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* cap, const int32_t* need,
                            const int32_t* rule_flags, const int32_t* truth, int64_t P, int32_t B, int64_t N, int64_t p_offset, int order,
                            int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind, int64_t* tie_class_hits_out,
                            int64_t* token_sum_out, int64_t* vote_count_sum_out, int64_t* truth_count_sum_out, int64_t* stop_hist_out,
                            int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out, int32_t* cell_votes_out) {
    return guarded([&]() -> int {
        const char* cells_given = (cells_out || cell_tokens_out || cell_votes_out) ? "cells_out / cell_tokens_out / cell_votes_out" : nullptr;
        if (int rc = check_lane_call("adaptive", ctx, P, B, N, p_offset, order, r_begin, r_end, cells_given, per_resample_out, M, mem_kind, no_check, [&] {
                if (!cap || !need || !tie_class_hits_out) return fail(SCV_ERR_ARG, "adaptive: cap, need and tie_class_hits_out are required");
                if (P > 0 && (!pool || !truth)) return fail(SCV_ERR_ARG, "adaptive: pool and truth are required");
                if ((token_sum_out || cell_tokens_out) && !tokens) return fail(SCV_ERR_ARG, "adaptive: token_sum_out / cell_tokens_out need tokens");
                return SCV_OK;
            })) return rc;
        if (mem_kind == SCV_MEM_HOST && rule_flags)                                // (DEVICE mode: the kernel checks, error bit 6 at scv_sync)
            for (int32_t b = 0; b < B; ++b)
                if (rule_flags[b] & ~(int32_t)SCV_STOP_DECIDED) return fail(SCV_ERR_ARG, "adaptive: rule_flags[%d] = 0x%x has a bit other than SCV_STOP_DECIDED", b, (unsigned)rule_flags[b]);
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_adaptive(ctx, pool, tokens, cap, need, rule_flags, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M,
                                   tie_class_hits_out, token_sum_out, vote_count_sum_out, truth_count_sum_out, stop_hist_out, per_resample_out,
                                   cells_out, cell_tokens_out, cell_votes_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t), rules = (size_t)B * sizeof(int32_t);
        enum { POOL, TOK, TRUTH, CAP, FLAGS, NEED, CELLS, CTOK, CVOTES, TIE, TSUM, VSUM, TCS, HIST, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(cap, rules), once_in(rule_flags, rules),
                       once_in(need, rules * (N + 1)), rows_out(cells_out, (size_t)B * sizeof(scv_cell)), rows_out(cell_tokens_out, sums),
                       rows_out(cell_votes_out, rules), sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums),
                       sums_out(vote_count_sum_out, sums), sums_out(truth_count_sum_out, sums), sums_out(stop_hist_out, sums * (N + 1)),
                       sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing voted, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {
            return launch_adaptive(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[CAP].at<const int32_t>(),
                                   rg[NEED].at<const int32_t>(), rg[FLAGS].at<const int32_t>(), rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0,
                                   order, r_begin, r_end, seed, M, rg[TIE].at<int64_t>(), rg[TSUM].at<int64_t>(), rg[VSUM].at<int64_t>(),
                                   rg[TCS].at<int64_t>(), rg[HIST].at<int64_t>(), rg[PER].at<int64_t>(), rg[CELLS].at<scv_cell>(),
                                   rg[CTOK].at<int64_t>(), rg[CVOTES].at<int32_t>(), err);
        });
    });
}

int scv_shortest_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* m_keep,
                            const int32_t* truth, int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin, int32_t r_end,
                            uint64_t seed, int32_t M, int mem_kind, int64_t* tie_class_hits_out, int64_t* voted_token_sum_out,
                            int64_t* spent_token_sum_out, int64_t* latency_sum_out, int64_t* truth_count_sum_out, int64_t* per_resample_out,
                            scv_cell* cells_out, int64_t* cell_tokens_out) {
    return guarded([&]() -> int {
        const char* cells_given = (cells_out || cell_tokens_out) ? "cells_out / cell_tokens_out" : nullptr;
        if (int rc = check_lane_call("shortest", ctx, P, B, N, p_offset, order, r_begin, r_end, cells_given, per_resample_out, M, mem_kind, no_check, [&] {
                if (!n_valid || !m_keep || !tie_class_hits_out) return fail(SCV_ERR_ARG, "shortest: n_valid, m_keep and tie_class_hits_out are required");
                if (P > 0 && (!pool || !tokens || !truth)) return fail(SCV_ERR_ARG, "shortest: pool, tokens and truth are required");
                return SCV_OK;
            })) return rc;
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_shortest(ctx, pool, tokens, n_valid, m_keep, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M, tie_class_hits_out,
                                   voted_token_sum_out, spent_token_sum_out, latency_sum_out, truth_count_sum_out, per_resample_out, cells_out,
                                   cell_tokens_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t), budgets = (size_t)B * sizeof(int32_t);
        enum { POOL, TOK, TRUTH, NV, MK, CELLS, CTOK, TIE, VSUM, SSUM, LSUM, TCS, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(n_valid, budgets), once_in(m_keep, budgets),
                       rows_out(cells_out, (size_t)B * sizeof(scv_cell)), rows_out(cell_tokens_out, sums),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(voted_token_sum_out, sums), sums_out(spent_token_sum_out, sums),
                       sums_out(latency_sum_out, sums), sums_out(truth_count_sum_out, sums),
                       sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing voted, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {
            return launch_shortest(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[NV].at<const int32_t>(),
                                   rg[MK].at<const int32_t>(), rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, order, r_begin, r_end, seed, M,
                                   rg[TIE].at<int64_t>(), rg[VSUM].at<int64_t>(), rg[SSUM].at<int64_t>(), rg[LSUM].at<int64_t>(),
                                   rg[TCS].at<int64_t>(), rg[PER].at<int64_t>(), rg[CELLS].at<scv_cell>(), rg[CTOK].at<int64_t>(), err);
        });
    });
}

int scv_iid_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_draws, const int32_t* truth,
                       int64_t P, int32_t B, int64_t N, int64_t p_offset, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                       int mem_kind, int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* truth_count_sum_out,
                       int64_t* per_resample_out) {
    return guarded([&]() -> int {
        if (int rc = check_lane_call("iid", ctx, P, B, N, p_offset, SCV_ORDER_SHUFFLED, r_begin, r_end, nullptr, per_resample_out, M, mem_kind, no_check, [&] {
                if (!n_draws || !tie_class_hits_out) return fail(SCV_ERR_ARG, "iid: n_draws and tie_class_hits_out are required");
                if (P > 0 && (!pool || !truth)) return fail(SCV_ERR_ARG, "iid: pool and truth are required");
                if (token_sum_out && !tokens) return fail(SCV_ERR_ARG, "iid: token_sum_out needs tokens");
                return SCV_OK;
            })) return rc;
        if (mem_kind == SCV_MEM_HOST)                                              // (DEVICE mode: the kernel checks, error bit 7 at scv_sync)
            for (int32_t b = 0; b < B; ++b)
                if (n_draws[b] > SCV_IID_MAX_DRAWS) return fail(SCV_ERR_ARG, "iid: n_draws[%d] = %d is above SCV_IID_MAX_DRAWS = %d", b, n_draws[b], SCV_IID_MAX_DRAWS);
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_iid(ctx, pool, tokens, n_draws, truth, P, B, N, p_offset, r_begin, r_end, seed, M, tie_class_hits_out, token_sum_out,
                              truth_count_sum_out, per_resample_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t);
        enum { POOL, TOK, TRUTH, ND, TIE, TSUM, TCS, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(n_draws, (size_t)B * sizeof(int32_t)),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums), sums_out(truth_count_sum_out, sums),
                       sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing drawn, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {
            return launch_iid(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[ND].at<const int32_t>(),
                              rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, r_begin, r_end, seed, M, rg[TIE].at<int64_t>(),
                              rg[TSUM].at<int64_t>(), rg[TCS].at<int64_t>(), rg[PER].at<int64_t>(), err);
        });
    });
}

int scv_resample_wide_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int32_t* n_valid, const int32_t* truth,
                          int64_t P, int32_t B, int64_t N, int64_t p_offset, int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                          int mem_kind, int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* truth_count_sum_out,
                          int64_t* per_resample_out) {
    return guarded([&]() -> int {
        if (int rc = check_lane_call("resample_wide", ctx, P, B, N, p_offset, SCV_ORDER_SHUFFLED, r_begin, r_end, nullptr, per_resample_out, M, mem_kind, no_check, [&] {
                if (!n_valid || !tie_class_hits_out) return fail(SCV_ERR_ARG, "resample_wide: n_valid and tie_class_hits_out are required");
                if (P > 0 && (!pool || !truth)) return fail(SCV_ERR_ARG, "resample_wide: pool and truth are required");
                if (token_sum_out && !tokens) return fail(SCV_ERR_ARG, "resample_wide: token_sum_out needs tokens");
                return SCV_OK;
            }, SCV_WIDE_MAX_N)) return rc;
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_wide(ctx, pool, tokens, n_valid, truth, P, B, N, p_offset, r_begin, r_end, seed, M, tie_class_hits_out, token_sum_out,
                               truth_count_sum_out, per_resample_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t);
        enum { POOL, TOK, TRUTH, NV, TIE, TSUM, TCS, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(n_valid, (size_t)B * sizeof(int32_t)),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums), sums_out(truth_count_sum_out, sums),
                       sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing drawn, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {     // (sums add: chunks of problems)
            return launch_wide(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[NV].at<const int32_t>(),
                               rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, r_begin, r_end, seed, M, rg[TIE].at<int64_t>(),
                               rg[TSUM].at<int64_t>(), rg[TCS].at<int64_t>(), rg[PER].at<int64_t>(), err);
        });
    });
}

int scv_token_budget_wide_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens, const int64_t* token_budget, const int32_t* truth,
                              int64_t P, int32_t B, int64_t N, int64_t p_offset, int order, int32_t r_begin, int32_t r_end, uint64_t seed,
                              int32_t M, int mem_kind, int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* vote_count_sum_out,
                              int64_t* truth_count_sum_out, int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out) {
    return guarded([&]() -> int {
        const char* cells_given = (cells_out || cell_tokens_out) ? "cells_out / cell_tokens_out" : nullptr;
        if (int rc = check_lane_call("token_budget_wide", ctx, P, B, N, p_offset, order, r_begin, r_end, cells_given, per_resample_out, M, mem_kind, no_check, [&] {
                if (!token_budget || !tie_class_hits_out) return fail(SCV_ERR_ARG, "token_budget_wide: token_budget and tie_class_hits_out are required");
                if (P > 0 && (!pool || !tokens || !truth)) return fail(SCV_ERR_ARG, "token_budget_wide: pool, tokens and truth are required");
                return SCV_OK;
            }, SCV_WIDE_MAX_N)) return rc;
        SCV_ENTER(ctx);
        if (!per_resample_out) M = 1;
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_wide_budget(ctx, pool, tokens, token_budget, truth, P, B, N, p_offset, order, r_begin, r_end, seed, M,
                                      tie_class_hits_out, token_sum_out, vote_count_sum_out, truth_count_sum_out, per_resample_out, cells_out,
                                      cell_tokens_out, ctx->d_err);
        const size_t row = (size_t)N * sizeof(int32_t), sums = (size_t)B * sizeof(int64_t);
        enum { POOL, TOK, TRUTH, BUD, CELLS, CTOK, TIE, TSUM, VSUM, TCS, PER };
        Region rg[] = {rows_in(pool, row), rows_in(tokens, row), rows_in(truth, sizeof(int32_t)), once_in(token_budget, (size_t)B * sizeof(int64_t)),
                       rows_out(cells_out, (size_t)B * sizeof(scv_cell)), rows_out(cell_tokens_out, sums),
                       sums_out(tie_class_hits_out, sums * SCV_TIE_CLASSES), sums_out(token_sum_out, sums), sums_out(vote_count_sum_out, sums),
                       sums_out(truth_count_sum_out, sums), sums_out(per_resample_out, (size_t)(r_end - r_begin) * M * sums)};
        if (P == 0 || r_end == r_begin) return zero_outputs(rg, PER + 1, P);       // HOST mode overwrites: nothing voted, all zero
        return stage_call(ctx, rg, PER + 1, P, kStageChunkBytes, [&](int64_t np, int64_t p0, uint32_t* err) {     // (sums add: chunks of problems)
            return launch_wide_budget(ctx, rg[POOL].at<const int32_t>(), rg[TOK].at<const int32_t>(), rg[BUD].at<const int64_t>(),
                                      rg[TRUTH].at<const int32_t>(), np, B, N, p_offset + p0, order, r_begin, r_end, seed, M, rg[TIE].at<int64_t>(),
                                      rg[TSUM].at<int64_t>(), rg[VSUM].at<int64_t>(), rg[TCS].at<int64_t>(), rg[PER].at<int64_t>(),
                                      rg[CELLS].at<scv_cell>(), rg[CTOK].at<int64_t>(), err);
        });
    });
}

int scv_expected_majority_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* n_valid, const int32_t* truth, int64_t P, int32_t B,
                              int64_t N, int mem_kind, double* expected_score_out, double* hit_prob_out) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        if (N < 1 || N > scv::kResampleMaxN || B < 1 || B > scv::kResampleMaxB || P < 0 || P > (1ll << 40))
            return fail(SCV_ERR_ARG, "expected_majority: bad shape P=%lld B=%d N=%lld (1 <= N <= %d, 1 <= B <= %d, P >= 0)",
                        (long long)P, B, (long long)N, scv::kResampleMaxN, scv::kResampleMaxB);
        if (!n_valid || !expected_score_out) return fail(SCV_ERR_ARG, "expected_majority: n_valid and expected_score_out are required");
        if (P > 0 && (!pool || !truth)) return fail(SCV_ERR_ARG, "expected_majority: pool and truth are required");
        if (mem_kind != SCV_MEM_HOST && mem_kind != SCV_MEM_DEVICE) return fail(SCV_ERR_ARG, "bad mem_kind %d", mem_kind);
        if (P == 0) return SCV_OK;
        SCV_ENTER(ctx);
        if (mem_kind == SCV_MEM_DEVICE)
            return launch_expected(ctx, pool, n_valid, truth, P, B, N, expected_score_out, hit_prob_out, ctx->d_err);
        enum { POOL, TRUTH, NV, SCORE, HIT };
        Region rg[] = {rows_in(pool, (size_t)N * sizeof(int32_t)), rows_in(truth, sizeof(int32_t)), once_in(n_valid, (size_t)B * sizeof(int32_t)),
                       rows_out(expected_score_out, (size_t)B * sizeof(double)), rows_out(hit_prob_out, (size_t)B * sizeof(double))};
        return stage_call(ctx, rg, HIT + 1, P, kStageChunkBytes, [&](int64_t np, int64_t, uint32_t* err) {
            return launch_expected(ctx, rg[POOL].at<const int32_t>(), rg[NV].at<const int32_t>(), rg[TRUTH].at<const int32_t>(), np, B, N,
                                   rg[SCORE].at<double>(), rg[HIT].at<double>(), err);
        });
    });
}

int scv_synth_fill_i32(scv_ctx* ctx, int32_t* answers, int32_t* tokens, int32_t* truth, int64_t P, int32_t B,
                       int64_t N, int64_t p_offset, uint64_t seed, int dist) {
    return guarded([&]() -> int {
        if (!ctx) return fail(SCV_ERR_ARG, "ctx is NULL");
        if (P < 0 || B < 0 || N < 0 || p_offset < 0) return fail(SCV_ERR_ARG, "synth_fill: negative shape");
        if (dist < SCV_DIST_UNIFORM || dist > SCV_DIST_DEGENERATE_WRONG) return fail(SCV_ERR_ARG, "synth_fill: unknown dist %d", dist);
        SCV_ENTER(ctx);
        if (P == 0) return SCV_OK;
        int64_t grid = P * (int64_t)B;
        if (B == 0) grid = (P + 255) / 256;
        const int64_t cap = (int64_t)ctx->num_cus * 16;
        if (grid > cap) grid = cap;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL(scv::scv_synth_fill_k, dim3((unsigned)grid), dim3(256), 0, ctx->stream, answers, tokens, truth, P,
                           B, N, p_offset, seed, dist);
        SCV_HIP(hipGetLastError());
        return SCV_OK;
    });
}

int scv_export_error_word(scv_ctx* ctx, int64_t* dst_device) {
    return guarded([&]() -> int {
        if (!ctx || !dst_device) return fail(SCV_ERR_ARG, "NULL argument");
        SCV_ENTER(ctx);
        // the word as scv_sync would JUDGE it: under SCV_FLAG_CLAMP_TO_INVALID_BIN an out-of-domain vote is not an error (bit 0 dropped)
        const uint32_t mask = (ctx->flags & SCV_FLAG_CLAMP_TO_INVALID_BIN) ? ~1u : ~0u;
        hipLaunchKernelGGL(scv::scv_export_err_k, dim3(1), dim3(1), 0, ctx->stream, ctx->d_err, mask, reinterpret_cast<long long*>(dst_device));
        SCV_HIP(hipGetLastError());
        return SCV_OK;
    });
}

int scv_last_kernel_ns(scv_ctx* ctx, uint64_t* ns_out) {
    return guarded([&]() -> int {
        if (!ctx || !ns_out) return fail(SCV_ERR_ARG, "NULL argument");
        if (!(ctx->flags & SCV_FLAG_TIMING) || ctx->events_used == 0)
            return fail(SCV_ERR_NOT_TIMED, "no timed launch (create the ctx with SCV_FLAG_TIMING)");
        SCV_ENTER(ctx);
        EventPair& ev = ctx->events[ctx->events_used - 1];
        SCV_HIP(hipEventSynchronize(ev.b));
        float ms = 0.f;
        SCV_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        *ns_out = (uint64_t)((double)ms * 1e6);
        return SCV_OK;
    });
}

int scv_drain_kernel_ns(scv_ctx* ctx, uint64_t* total_ns_out, uint64_t* launches_out) {
    return guarded([&]() -> int {
        if (!ctx || !total_ns_out || !launches_out) return fail(SCV_ERR_ARG, "NULL argument");
        if (!(ctx->flags & SCV_FLAG_TIMING)) return fail(SCV_ERR_NOT_TIMED, "ctx was created without SCV_FLAG_TIMING");
        SCV_ENTER(ctx);
        double total = 0;
        for (size_t i = 0; i < ctx->events_used; ++i) {
            SCV_HIP(hipEventSynchronize(ctx->events[i].b));
            float ms = 0.f;
            SCV_HIP(hipEventElapsedTime(&ms, ctx->events[i].a, ctx->events[i].b));
            total += (double)ms * 1e6;
        }
        *total_ns_out = (uint64_t)total;
        *launches_out = ctx->events_used;
        ctx->events_used = 0;
        return SCV_OK;
    });
}

int scv_host_alloc(void** out, size_t bytes) {
    return guarded([&]() -> int {
        if (!out) return fail(SCV_ERR_ARG, "scv_host_alloc: out is NULL");
        *out = nullptr;
        if (bytes == 0) return SCV_OK;
        SCV_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
        return SCV_OK;
    });
}

int scv_host_free(void* p) {
    return guarded([&]() -> int {
        if (!p) return SCV_OK;
        SCV_HIP(hipHostFree(p));
        return SCV_OK;
    });
}

int scv_get_stat(scv_ctx* ctx, const char* key, int64_t* out) {
    return guarded([&]() -> int {
        if (!ctx || !key || !out) return fail(SCV_ERR_ARG, "NULL argument");
        if (!strcmp(key, "boot_fused")) *out = ctx->stat_boot_fused;
        else if (!strcmp(key, "boot_separate")) *out = ctx->stat_boot_separate;
        else if (!strcmp(key, "boot_recovered")) *out = ctx->stat_boot_recovered;
        else if (!strcmp(key, "boot_cooperative")) *out = ctx->stat_boot_cooperative;
        else if (!strcmp(key, "overwrite_fused")) *out = ctx->stat_overwrite_fused;
        else if (!strcmp(key, "lds_counters")) *out = ctx->stat_lds_counters;
        else if (!strcmp(key, "prefix_cells")) *out = ctx->stat_prefix_cells;
        else if (!strcmp(key, "prefix_lane")) *out = ctx->stat_prefix_lane;
    else if (!strcmp(key, "prefix_pool")) *out = ctx->stat_prefix_pool;
    else if (!strcmp(key, "prefix_sort")) *out = ctx->stat_prefix_sort;
    else if (!strcmp(key, "prefix_tokens")) *out = ctx->stat_prefix_tokens;
    else if (!strcmp(key, "one_vote")) *out = ctx->stat_one_vote;
        else if (!strcmp(key, "sort_cells")) *out = ctx->stat_sort_cells;
        else if (!strcmp(key, "few_votes")) *out = ctx->stat_few_votes;
        else if (!strcmp(key, "host_small_calls")) *out = ctx->stat_small_calls;
        else if (!strcmp(key, "host_pipelined_calls")) *out = ctx->stat_pipelined_calls;
        else if (!strcmp(key, "resample_calls")) *out = ctx->stat_resample_calls;
        else if (!strcmp(key, "expected_calls")) *out = ctx->stat_expected_calls;
        else if (!strcmp(key, "token_budget_calls")) *out = ctx->stat_token_budget_calls;
        else if (!strcmp(key, "host_thread_start_failures")) *out = ctx->pipe ? ctx->pipe->pool.start_failures : 0;
        else return fail(SCV_ERR_ARG, "unknown stat '%s'", key);
        return SCV_OK;
    });
}

int scv_device_info(scv_ctx* ctx, int64_t info_out[4]) {
    return guarded([&]() -> int {
        if (!ctx || !info_out) return fail(SCV_ERR_ARG, "NULL argument");
        info_out[0] = ctx->num_cus;
        info_out[1] = ctx->lds_max;
        info_out[2] = ctx->clock_khz;
        info_out[3] = ctx->hbm_bytes;
        return SCV_OK;
    });
}

}  // extern "C"

// ---- what csrc/scvote_comm.hip needs of the opaque context -----------------------------------------------------------
namespace scv {
hipStream_t ctx_stream(scv_ctx* ctx) { return ctx->stream; }
int ctx_device(scv_ctx* ctx) { return ctx->device; }
int comm_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace scv

// ---- kernel tables: the per-translation-unit tables behind one switch each (scvote_dispatch.h) ----------------------
namespace scv {
KernelFn pick_kernel(int copies, int t, int u, bool tok, bool xtra) {
    switch (copies) {
    case 4: return pick_stream_c4(t, u, tok, xtra);
    case 8: return pick_stream_c8(t, u, tok, xtra);
    case 16: return pick_stream_c16(t, u, tok, xtra);
    default: return nullptr;
    }
}
RegKernel pick_reg_kernel(int g, int v, bool tok, bool vec) {
    if (g == 8) return pick_reg_g8(v, tok, vec);
    if (g == 16) return pick_reg_g16(v, tok, vec);
    if (g == 32) return pick_reg_g32(v, tok, vec);
    return pick_reg_g64(v, tok, vec);
}
}  // namespace scv
