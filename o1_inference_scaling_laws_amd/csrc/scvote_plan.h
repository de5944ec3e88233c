// scvote_plan.h -- the DECISIONS of the dense and prefix aggregate dispatch (scvote.hip: launch_aggregate, launch_prefix) as pure functions of the shape and
// of an options struct that scvote.hip fills from the context: which kernel serves which N, which register shape, how many segments, how much LDS.  Plain
// C++17, no HIP and no context in it: tests/plan_check.cpp prints the answers on the CPU and tests/test_dispatch_plan_cpu.py states what they must be.
// Where a decision needs the runtime's occupancy answer, that answer is an argument; the query itself stays in scvote.hip.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace scv {
namespace plan {

// restated from scvote_kernels.hip.h / include/scvote.h (scvote.hip static_asserts that they agree)
constexpr int kBins = 1024, kRedWords = 96, kMaxSortedB = 512, kSplitTickets = 512, kCellBytes = 16;
constexpr size_t kLaneLdsMax = (size_t)60 * 1024;      // LDS tables of the one-lane-per-cell kernels: above, another kernel takes the call

struct Options {
    int path, prefix_path, tiny_n_max, reg_n_max, sort_n_max, sort_n_min, reg_shape, fused_counters_max, overwrite_counters, segs_override, split_seg_kb;
    int copies, threads, wg_per_cu, unroll; bool user_tuned;      // scv_set_tuning
    int num_cus; int64_t lds_max;
};

// ---- vote-count roundings: the NV of the kernel instantiation that takes N votes ---------------------------------------------------
inline int lane_nv(int64_t N) { return N <= 4 ? 4 : (N <= 8 ? 8 : (N <= 16 ? 16 : 32)); }                       // scv_lane_cells
inline int prefix_lane_nv(int64_t N) { return N <= 32 ? lane_nv(N) : 64; }                                      // scv_lane_prefix
inline int sort_nv(int64_t N) { return N <= 8 ? 8 : (N <= 16 ? 16 : (N <= 24 ? 24 : (N <= 32 ? 32 : (N <= 40 ? 40 : (N <= 48 ? 48 : (N <= 56 ? 56 : 64)))))); }   // scv_sort_cells
inline int sort_prefix_nv(int64_t N) { return N <= 32 ? 32 : (N <= 64 ? 64 : 128); }                           // scv_sort_prefix / scv_sort_prefix2
// lds bytes of the one-lane-per-cell kernel (tie classes 0..nv and two sums per budget)
inline size_t lane_kernel_lds(int32_t B, int nv) { return (((size_t)B * (nv + 1) + 1) & ~(size_t)1) * sizeof(uint32_t) + 2 * (size_t)B * sizeof(unsigned long long); }
inline bool lane_tables_fit(int32_t B, int64_t N) { return lane_kernel_lds(B, lane_nv(N)) <= kLaneLdsMax; }

// ---- which kernel serves a dense or pool-rows call (auto-selected from the shape; the "path" option forces one) ------------------------
//   lane      N <= 4 (and pool rows <= 32)  one lane per cell, registers only                (scv_lane_cells)
//   sorted    5 / 8 <= N <= 64              one lane per cell, rows by LDS-DMA, sorted       (scv_sort_cells)
//   register  up to 8192                    a cell in the registers of 16 / 32 / 64 lanes    (scv_reg_cells, scv_reg_dense)
//   stream    everything else               one persistent workgroup streams whole cells, or -- cells <= CUs/2, big N -- several workgroups per
//                                           cell, merged in the launch (scv_hist_argmax)
enum Kind { LANE, SORT, REG, STREAM };
inline Kind cell_kind(const Options& o, int64_t N, int32_t B, bool rows_aligned, bool tok, bool pool_rows) {
    const int64_t Nreg = rows_aligned ? N : N + 3;      // register-resident kernels read unaligned rows as their aligned supersets
    const bool sort_ok = !pool_rows && o.sort_n_max > 0 && N >= (rows_aligned ? 4 : 1) && N <= (o.sort_n_max < 64 ? o.sort_n_max : 64);
    Kind kind;
    if (o.path == 5) kind = sort_ok ? SORT : (N <= o.tiny_n_max ? LANE : (Nreg <= 8192 ? REG : STREAM));
    else if (o.path == 4) kind = (Nreg <= 8192 && N >= 1) ? REG : STREAM;
    else if (o.path >= 1 && o.path <= 3) kind = STREAM;
    else if (sort_ok && N >= (rows_aligned ? o.sort_n_min : (o.sort_n_min < 5 ? o.sort_n_min : 5))) kind = SORT;
    else if (N <= o.tiny_n_max) kind = LANE;
    else if (N <= o.reg_n_max && Nreg <= 8192) kind = REG;
    else kind = STREAM;
    if (kind == LANE && !lane_tables_fit(B, N)) kind = REG;   // (thousands of budgets)
    // 17 .. 32 votes with tokens on one lane per cell need 256 VGPRs + scratch at 512 threads (pool rows / sorted cells switched off
    // only -- dense cells of this length are sorted): the register-resident shape of 64 votes takes them
    if (kind == LANE && tok && N > 16) kind = REG;
    return kind;
}
// the sorted-cells launch did not fit the LDS (hundreds of budgets): who takes the call instead
inline Kind sort_fallback_kind(const Options& o, int64_t N, int32_t B) { return N <= o.tiny_n_max && lane_tables_fit(B, N) ? LANE : REG; }

// ---- per-budget counters: inside the launch (LDS tables of the cell kernels; per-cell atomics of the streaming kernel for few cells, or when a
// row is >= 4 MiB) or from the cell table by scv_reduce_cells (same-address device atomics serialise at ~12 ns each; measured,
// profiles/r01_crossover_r4_d1.log: 65536 cells of 64 KiB with fused atomics 4.1 TB/s, with the separate reduction 6.6)
inline bool counters_by_reduce(const Options& o, bool want_counters, bool streaming, int64_t ncells, int32_t B, int64_t N) {
    return want_counters && (o.fused_counters_max == 0 || (streaming && ncells > o.fused_counters_max && N * (int64_t)B < (1 << 20)));
}
// Option "overwrite_counters": the streaming kernel turns its cell table into the counters with its last workgroup (single launch: no memset, no
// reduce launch) when the cells are few, whole (S == 1) and the geometry has the epilogue variant; every other launch gets memset nodes in front and
// accumulates -- a streaming call of few cells INSIDE the launch whatever fused_counters_max says.
inline bool overwrite_few_cells(const Options& o, bool want_counters, int64_t ncells, int32_t B) { return o.overwrite_counters && want_counters && ncells <= 8192 && B <= 64; }
// chunks of problems per budget of scv_reduce_cells (grid.x)
inline int64_t reduce_chunks(int64_t P, int32_t B, int num_cus) {
    const int64_t chunks = (P + 2047) / 2048, cap = ((int64_t)num_cus * 8 + B - 1) / B;
    return std::max<int64_t>(1, std::min(chunks, cap));
}
// Tie classes per budget in the LDS the resident workgroups leave free ([B][TCL] + 2 B sums per workgroup, flushed by the same launch); 0: none.
// TCL < min(N, 1024) + 1 only with many budgets: the classes that do not fit go to memory directly, and below 8 it is not worth it.
inline int64_t lds_tie_classes(int64_t spare_words, int32_t B, int64_t N) {
    const int64_t full = (N < 1024 ? N : 1024) + 1;
    int64_t tcl = spare_words > 4 * (int64_t)B + 2 ? (spare_words - 4 * (int64_t)B - 2) / B : 0;
    if (tcl > full) tcl = full;
    return (tcl >= 8 || tcl == full) ? tcl : 0;
}
inline size_t tie_classes_lds(int32_t B, int64_t tcl) { return ((((size_t)B * tcl + 1) & ~(size_t)1) + 4 * (size_t)B) * sizeof(uint32_t); }
inline int64_t nv_cache_words(bool has_n_valid, int32_t B) { return has_n_valid && B <= kMaxSortedB ? ((B + 3) & ~3) : 0; }   // the n_valid cache of the cell kernels
// cells per grid step a multiple of B: every lane slot then sees one budget and keeps its counters in registers
inline int64_t b_multiple_grid(int64_t grid, int64_t cells_per_wg, int32_t B) { return ((grid * cells_per_wg) % B != 0 && grid > B) ? grid - grid % B : grid; }

// ---- cells of exactly 1, 2 or 4 votes (the reference's most common sizes, o1.py:276,302): a block of 256 / 128 / 64 cells per wave and step, 1024
// threads.  ok: the few-votes kernels take the call (else scv_lane_cells); one: the kernel whose loop body is one compare per cell (N = 1: scv_one_vote;
// N = 2, o1.py:276 at T = 4096: scv_two_votes, blocks of 128 cells) -- when the grid step is a multiple of B (it is, unless the launch is smaller than B
// workgroups or the grid is forced); it also takes the cells behind the last whole block (large launches only: a few hundred cells are the general kernel's)
struct FewVotes { bool ok, one; int64_t grid; };
inline FewVotes few_votes(const Options& o, int64_t N, int32_t B, int64_t ncells, bool bases_aligned, bool pool_rows, int grid_override) {
    FewVotes f{false, false, 0};
    if (!((N == 1 || N == 2 || N == 4) && !pool_rows && ncells < (1ll << 29) && bases_aligned && lane_kernel_lds(B, (int)N) <= kLaneLdsMax)) return f;
    const int64_t nblocks = ncells / (256 / N), waves = 1024 / 64;      // whole blocks
    // two workgroups per CU: 32 waves, each with a block in flight behind the one it counts
    const int64_t grid = std::max<int64_t>(1, std::min((nblocks + waves - 1) / waves, (int64_t)o.num_cus * 2));
    f.grid = grid_override > 0 ? grid_override : b_multiple_grid(grid, waves * (256 / N), B);
    f.one = N <= 2 && (f.grid * waves * (256 / N)) % B == 0 && (size_t)B * 32 <= kLaneLdsMax && (ncells % (256 / N) == 0 || ncells >= 65536);
    f.ok = f.one || ncells % (256 / N) == 0;
    return f;
}
// one lane per cell (scv_lane_cells): threads by the register budget (2 x nv votes (+ tokens) per lane), one workgroup per CU (the flush costs one
// atomic per workgroup and counter), grid * threads a multiple of B
inline int64_t lane_grid(const Options& o, int64_t ncells, int nv, bool tok, int32_t B) {
    const int threads = (nv == 32 || (nv == 16 && tok)) ? 512 : 1024;
    return b_multiple_grid(std::min<int64_t>((ncells + threads - 1) / threads, o.num_cus), threads, B);
}

// ---- register-resident cells: shape of the kernel from the slots a row needs (N, or N + 3 for unaligned rows); the "reg_shape" option forces one for
// A/B runs: g*100 + v (sparse: g lanes per cell, v vectors per lane) or 1000 + v*10 + h (dense: h parts of v vectors).
// have_g8: the forced (8, v) shape is instantiated (scvote_dispatch.h pick_reg_g8; (8, 4): A/B builds only)
struct RegShape { int g, v, h; };
inline RegShape reg_shape(int64_t Nreg, int forced, bool have_g8) {
    int g = 0, v = 4, h = 0;
    if (Nreg <= 64) { g = 16; v = 1; }
    else if (Nreg <= 96) { g = 8; v = 3; }        // round 6: 96 slots for 65 ... 96 votes (8 lanes x 3 vectors, 8-bit bins), not 128 ("reg_shape" = 1602: round 5's shape)
    else if (Nreg <= 128) g = 8;                  // ... and 8 lanes x 4 vectors for 97 ... 128 (3-10 % over 16 lanes x 2: eight cells per wave share the fixed work)
    else if (Nreg <= 256) g = 16;
    else if (Nreg <= 512) g = 32;
    else if (Nreg <= 896) g = 64;
    else if (Nreg <= 1024) h = 1;                 // round 3 (with the pivots): one dense part beats the sparse read-back from ~900 votes (N = 1024: 189 vs 200 us; 768: 224 vs 215)
    else if (Nreg <= 2048) h = 2;                 // 4 KiB parts: 126-136 VGPRs, 3 waves per SIMD (8 KiB parts: 200, 2 waves; measured 73 vs 79 us)
    else if (Nreg <= 4096) h = 4;
    else h = 8;                                   // 4096 < N <= 8192: 4.5 -> 5.4 TB/s at N = 4608 against the streaming kernel, equal at 8192
    // (the dense codes are 1041 ... 1048 ONLY: 1601 / 1602 / 1604 / 3204 / 6404 are sparse shapes)
    if (forced >= 1040 && forced < 1050) {
        const int fv = (forced - 1000) / 10, fh = forced % 10;
        if (fv == 4 && (fh == 1 || fh == 2 || fh == 4 || fh == 8) && (int64_t)256 * fv * fh >= Nreg) { g = 0; v = fv; h = fh; }
    } else if (forced > 0) {
        const int fg = forced / 100, fv = forced % 100;
        const bool have = (fg == 16 && (fv == 1 || fv == 2 || fv == 4)) || ((fg == 32 || fg == 64) && fv == 4) || (fg == 8 && (fv == 3 || fv == 4));
        if (have && (int64_t)4 * fg * fv >= Nreg && (fg != 8 || have_g8)) { g = fg; v = fv; h = 0; }
    }
    return RegShape{g, v, h};
}
// SCV_FLAG_PACKED_CELLS: the kernels that write the 4-byte record (they call pack_cell, scvote_kernels.hip.h / scvote_sort.hip.h): one lane per cell
// (scv_lane_cells, scv_few_votes, scv_one_vote, scv_two_votes), sorted cells (scv_sort_cells) and the SPARSE register-resident shapes (scv_reg_cells).
// The dense register-resident parts (scv_reg_dense) and the streaming kernel (scv_hist_argmax, and scv_reduce_cells reading its table) know 16-byte
// records only: a packed context with a cell table must not reach them (launch_cells refuses the call).  kind: the kernel that RUNS (behind
// sort_fallback_kind when the sorted launch does not fit); s: the register shape of the call (read for REG only).
inline bool packed_ok(Kind kind, const RegShape& s) { return kind == LANE || kind == SORT || (kind == REG && s.h == 0); }
// The grid is persistent, so it must not exceed what is resident at once (CUs x the runtime's occupancy answer, or the forced grid).  A wave strides over
// the batches by grid * WPG: keep the stride coprime with B so that every wave visits every budget (ragged n_valid would otherwise give some waves only the long budgets)
inline int64_t reg_grid(int64_t resident, int64_t nbatches, int WPG, int32_t B) {
    int64_t grid = resident;
    const int64_t wgs_needed = (nbatches + WPG - 1) / WPG;
    if (grid >= wgs_needed) return wgs_needed;
    auto gcd = [](int64_t x, int64_t y) { while (y) { const int64_t t = x % y; x = y; y = t; } return x; };
    while (grid > 1 && gcd(grid * WPG, B) != 1 && gcd(grid, B) != 1) --grid;
    return grid;
}

// ---- sorted cells: one region per wave (votes image | tokens image | the cells' truth values, 256 bytes) and the tables behind them -----
inline int64_t sort_region_words(int64_t N, bool tok, bool lin) {
    const int64_t image_words = lin ? ((64 * N * 4 + 16 + 1023) >> 10) * 256 : 64 * ((N / 4) | 1) * 4;
    return image_words * (tok ? 2 : 1) + 64;
}
inline int64_t sort_tail_words(bool has_n_valid, int32_t B, int nv) { return nv_cache_words(has_n_valid, B) + ((((int64_t)B * (nv + 1) + 1) & ~(int64_t)1) + 4 * (int64_t)B); }
// waves per workgroup of scv_sort_cells that fit the LDS; 0: the launch does not fit (sort_fallback_kind)
inline int sort_waves(int waves, int64_t region_words, int64_t tail_words, int64_t lds_max) {
    int W = waves;
    while (W > 1 && (W * region_words + tail_words) * 4 > lds_max) --W;
    // whole waves per SIMD: the steps are VALU-bound, so with 14 waves (N = 37 ... 44) two SIMDs carry 4 and set the pace of a round that 12 waves finish as
    // fast with the other two SIMDs idle a quarter of the time (N = 40 / 44 / 56: 72.1 / 72.7 / 82.4 -> 67.5 / 68.0 / 78.1 us, profiles/r06_sort_waves_ab.log);
    // not below 8: with tokens 7 / 6 / 5 waves beat 4 by 10-17 % (one wave per SIMD cannot hide its own copy)
    if (W > 8) W &= ~3;
    return ((W * region_words + tail_words) * 4 <= lds_max && W >= (waves >= 16 ? 4 : 2)) ? W : 0;
}
// sort-prefix: one image per wave (a step's tokens follow its votes through it; 128: the row goes through the image in two halves of up to 64 votes)
inline int64_t sort_prefix_region_words(int64_t N, int nv) { return 64 * (nv == 128 ? 17 : ((N / 4) | 1)) * 4 + 64; }
// waves per workgroup that fit; 0: none does.  tail_words: scv::sort_prefix_tail_words(nv, B) (scvote_dispatch.h)
inline int sort_prefix_waves(int waves, int64_t region_words, int64_t tail_words, int64_t lds_max) {
    int W = waves;
    while (W > 2 && (W * region_words + tail_words) * 4 + 1024 > lds_max) --W;
    return (W * region_words + tail_words) * 4 + 1024 > lds_max ? 0 : W;
}

// ---- streaming kernel geometry -------------------------------------------------------------------------------------------------------
struct StreamBand { int copies, threads, wg_per_cu, unroll; size_t lds; };
inline StreamBand stream_band(const Options& o, int64_t N, int64_t ncells) {
    StreamBand b{o.copies, o.threads, o.wg_per_cu, o.unroll, 0};
    if (!o.user_tuned) {
        // measured crossover (tools/crossover.py): the per-cell fold costs 1024*R LDS words, so short
        // cells want small R and several cells in flight per CU; long cells want one big workgroup.
        if (N < 4096) b = StreamBand{4, 256, 8, 2, 0};            // latency-bound: most cells in flight
        else if (N < 32768) b = StreamBand{8, 256, 4, 4, 0};
        else if (N < 262144) b = StreamBand{16, 512, 2, 4, 0};
        else b = StreamBand{16, 1024, 1, 4, 0};
        // fewer cells than CUs: one cell per CU whatever the band, so give each the widest workgroup
        if (ncells <= o.num_cus && N >= 4096) b = StreamBand{16, 1024, 1, 4, 0};
    }
    b.lds = ((size_t)kBins * b.copies + kRedWords + kMaxSortedB) * sizeof(uint32_t);
    if ((int64_t)b.lds > o.lds_max) return b;          // (the caller refuses the request)
    const int by_lds = (int)((160 * 1024) / b.lds), by_waves = 2048 / b.threads;
    b.wg_per_cu = std::max(1, std::min({b.wg_per_cu, by_lds, by_waves}));
    return b;
}
// split-N when whole cells cannot fill the chip: S workgroups per cell.  Measured (tools/segs_sweep.py): best is ONE round of items (at most one per
// workgroup slot) -- more, smaller segments only add fold/publish/merge work.  Round 6: the segments of a cell are merged INSIDE the launch (device
// atomics into the cell's histogram in memory, the last segment to arrive runs the epilogue), so a segment costs its fold + 16 atomic instructions, not
// 4 KiB of traffic and a share of a second kernel: segments of 256 KiB, one round over every workgroup slot (a single cell of 2^24 votes: 128 x 512 KiB +
// merge launch = 27.8 us in round 5).  seg_len is a multiple of 4 votes: segments start 16-byte aligned in aligned rows.
struct Split { int64_t S, seg_len; };
inline Split split(const Options& o, int64_t N, int64_t ncells, int64_t slots) {
    int64_t S = 1;
    if ((o.path == 2 || (o.path == 0 && 2 * ncells <= slots && N * 4 >= (1 << 20))) && ncells <= kSplitTickets) {
        S = o.segs_override > 0 ? o.segs_override : std::min(slots / ncells, (N * 4) / (o.split_seg_kb << 10));
        S = std::max<int64_t>(1, std::min<int64_t>(S, 4096));
    }
    return Split{S, S > 1 ? (((N + S - 1) / S + 3) & ~(int64_t)3) : N};
}
// A 4 MiB cell is several percent of a launch: a ragged last round (10000 cells over 256 workgroups = 39.06 rounds) idles most of the chip for a whole
// cell.  Use the smallest grid with the same number of rounds, so every workgroup streams `rounds` (or rounds-1) items.
inline int64_t stream_grid(int64_t nitems, int64_t slots, int grid_override) {
    const int64_t grid = std::min<int64_t>(grid_override > 0 ? grid_override : slots, nitems);
    if (grid_override > 0) return grid;
    const int64_t rounds = (nitems + grid - 1) / grid;
    return (nitems + rounds - 1) / rounds;
}
// Dynamic items: the workgroups of a round-robin launch over 4 MiB cells finish up to ~10 % apart (more on some allocations), and the
// launch waits for the slowest; a counter that hands out the items lets the early finishers take more (profiles/r06_footprint_probe.log,
// r06_dynamic_items_ab.log).  Items of at least 2^20 votes -- the length it was measured at; option path = 3 keeps the round-robin order.
inline bool use_dispenser(const Options& o, int64_t nitems, int64_t grid, int64_t item_len) {
    return o.path != 3 && nitems > grid && nitems < ((int64_t)1 << 31) && item_len >= ((int64_t)1 << 20);
}

// ---- prefix budgets over one pool per problem ----------------------------------------------------------------------------------------
// Short pools (N <= 4096: the reference's own sizes) go through the cell kernels: the pool row is re-read per budget, but out of the cache, and a cell
// costs what its n_valid votes cost -- the one-pass streaming kernel pays a workgroup-wide fold per boundary (measured at P x N = 10^5 x 256, budgets
// 1, 2, 4 ... N: 240 -> 60 us).
inline bool pool_rows_eligible(const Options& o, int32_t B, int64_t N, bool rows_aligned) {
    if (o.path != 0 || N < 1) return false;
    if (N > o.tiny_n_max) return N <= o.reg_n_max && N + (rows_aligned ? 0 : 3) <= 4096;   // (+ 3: an unaligned pool row is read as its aligned superset)
    return lane_tables_fit(B, N);
}
// pools of up to 64 samples: scv_lane_prefix (tie classes 0..nv, two sums, order + sorted n_valid per budget in LDS; the snapshots of a wave's 64 x B cells
// staged in LDS: 16 bytes each, 24 with tokens -- budget lists whose snapshots do not fit even a 256-thread workgroup run on scv_prefix_pool, which holds
// one record per lane whatever the number of budgets)
struct PrefixLane { bool ok; int nv, threads; size_t lds, lds_total; };
inline PrefixLane prefix_lane(const Options& o, int32_t B, int64_t N, bool tok) {
    PrefixLane r{false, 0, 0, 0, 0};
    if (o.path != 0 || N < 1 || N > 64 || B > kMaxSortedB) return r;
    r.nv = prefix_lane_nv(N);
    r.lds = ((((size_t)B * (r.nv + 1) + 1) & ~(size_t)1) + 6 * (size_t)B) * sizeof(uint32_t);
    if (r.lds > (size_t)24 * 1024) return r;
    const size_t counters_bytes = (r.lds + 15) & ~(size_t)15, per_wave = (size_t)64 * B * (kCellBytes + (tok ? sizeof(int64_t) : 0));
    for (int t = r.nv == 64 ? 256 : 1024; t >= 256 && !r.ok; t >>= 1)
        if (counters_bytes + (size_t)(t / 64) * per_wave + 1024 <= (size_t)o.lds_max) r = PrefixLane{true, r.nv, t, r.lds, counters_bytes + (size_t)(t / 64) * per_wave};
    return r;
}
// budgets scv_sort_prefix serves: 0, a power of two <= np, or the whole row
inline int64_t sort_prefix_np(int64_t N) { return N <= 32 ? 16 : (N <= 64 ? 32 : 64); }
inline bool budget_served(int64_t n, int64_t N) { return n <= 0 || n >= N || ((n & (n - 1)) == 0 && n <= sort_prefix_np(N)); }
// pools of 17 .. 128 votes, budgets that are powers of two (the reference's own, o1.py:274-277): every budget out of one sort per problem.  Pools of
// 68 .. 128 votes (scv_sort_prefix2: two sorts, a merge and a 128-vote scan per step) pay ~27 us for a launch of one step per wave (36 before round 6's
// 4-wave workgroups): measured against scv_prefix_pool it wins from ~5e4 pools (4.9e4: 28.9 against 29.5 us, 6.6e4: 30.1 against 35.2, 2e5: 48 .. 63
// against 82; 3e4: 153 against 69 in HOST-mode chunks); with tokens (round 6) the sums come from token steps of the same launch (round 5 tried a second
// image: 114 against 114 us, and left such calls on scv_prefix_pool); prefix_path = 5 selects it for any number of pools
inline bool sort_prefix_eligible(const Options& o, int64_t P, int32_t B, int64_t N, bool rows_aligned) {
    return o.path == 0 && (o.prefix_path == 0 || o.prefix_path == 5) && o.sort_n_max >= 64 && o.fused_counters_max != 0 && rows_aligned &&
           N > 16 && N <= 128 && B <= kMaxSortedB && (N <= 64 || P >= 57344 || o.prefix_path == 5);
}
// which form serves a prefix call once the sort-prefix attempt is behind it (skip_sortable: scv_sort_prefix is queued in front)
enum PrefixForm { PREFIX_POOL, PREFIX_CELLS, PREFIX_LANE, PREFIX_HIST };
inline PrefixForm prefix_form(const Options& o, int32_t B, int64_t N, bool rows_aligned, bool lane_fits, bool skip_sortable) {
    const bool lane_ok = lane_fits && (o.prefix_path == 0 || o.prefix_path == 1 || o.prefix_path == 5);
    // pools of 65 .. 4096 votes (and shorter ones when forced): ONE pass per problem, every budget a snapshot (scv_prefix_pool)
    if (o.path == 0 && N >= 1 && N <= 4096 && B <= kMaxSortedB && (((o.prefix_path == 0 || o.prefix_path == 5) && !lane_ok) || o.prefix_path == 4)) return PREFIX_POOL;
    if (!lane_ok && !skip_sortable && pool_rows_eligible(o, B, N, rows_aligned) && (o.prefix_path == 0 || o.prefix_path == 2)) return PREFIX_CELLS;
    return lane_ok ? PREFIX_LANE : PREFIX_HIST;
}
// scv_prefix_pool, lanes per problem: 16 up to 1024 votes (4 problems per wave share the fixed work per boundary; 16-bit bins: 16 waves per CU), 32 beyond
// (measured: 1024 votes 68 us at 16 lanes against 82 at 32, 4096 votes 100 against 87); unaligned rows: 16 (the only unaligned shape: scvote_prefix.hip)
inline int prefix_pool_lanes(const Options& o, int64_t N, bool rows_aligned) {
    return !rows_aligned ? 16 : ((o.reg_shape == 16 || o.reg_shape == 32) ? o.reg_shape : (N <= 1024 ? 16 : 32));
}

}  // namespace plan
}  // namespace scv
