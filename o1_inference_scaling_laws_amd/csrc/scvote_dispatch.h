// scvote_dispatch.h -- host-side tables that map a launch geometry to a kernel instantiation.
//
// The kernel family is ~120 template instantiations.  They are spread over several translation units
// (scvote_stream_c{4,8,16}.hip: the streaming kernel by LDS replication; scvote_reg_g{8,16,32,64}.hip: register-resident
// cells by lanes per cell; scvote_dense.hip: register-streamed long cells; scvote_sort.hip: sorted cells) so that hipcc compiles
// them in parallel (_build.py) and an edit to one kernel rebuilds one table.  scvote.hip (the C ABI) only sees these prototypes.
#pragma once

#include "scvote_kernels.hip.h"
#include "scvote_expected_table.h"

namespace scv {

using KernelFn = void (*)(const AggArgs);
struct RegKernel { KernelFn fn; int waves; };   // + the workgroup size (waves) the kernel was compiled for

// Waves per workgroup of a one-wave-per-step kernel (scv_sort_cells, scv_sort_prefix, scv_sort_prefix2) when the launch has fewer steps than the chip
// has wave slots: every SIMD of a CU gets a wave before any gets a second one (two waves of a SIMD in the same VALU-bound step take turns: 4.9 against
// 3.0 us for the sort of a one-step launch of 64-vote pools) -- but never fewer than one wave per SIMD: every workgroup ends in one device atomic per
// counter word, ~13 ns each on ONE word whoever sends it (391 one-wave workgroups: 5 us of epilogue; 98 of four waves: 1.3; profiles/r06_sort_prefix_wall.log).
// Only while that at least halves the workgroup: 7 waves instead of 8 leave three SIMDs with two waves AND add workgroups (1e5 pools of 64 votes: 22.5 against 21.7 us).
// (least: 4 = one wave per SIMD; 8 for the cheap steps of scv_sort_cells<8 | 16>, where more workgroups cost more than shared SIMDs: 1000 steps of 16 votes 9.6 against 8.9 us)
inline int spread_waves(int64_t nsteps, int waves, int num_cus, int least = 4) {
    int w = (int)((nsteps + num_cus - 1) / num_cus);
    if (w < least) w = least;
    return 2 * w <= waves ? w : waves;
}

// streaming kernel scv_hist_argmax<log2(copies), threads, unroll, tokens, xtra>.  Instantiated geometries (copies, threads):
// (4, 256) (8, 256) (8, 512) (16, 256) (16, 512) (16, 1024), 4 loads in flight per lane ((4, 256): 2 -- the short-cell band);
// xtra (single-launch epilogues: overwrite-counters, bootstrap behind a grid barrier) for the four the library picks itself:
// (4, 256) (8, 256) (16, 512) (16, 1024).  NULL: not instantiated.
KernelFn pick_kernel(int copies, int threads, int unroll, bool tok, bool xtra);
KernelFn pick_stream_c4(int threads, int unroll, bool tok, bool xtra);
KernelFn pick_stream_c8(int threads, int unroll, bool tok, bool xtra);
KernelFn pick_stream_c16(int threads, int unroll, bool tok, bool xtra);

// scv_reg_cells<g lanes per cell, v vectors per lane, ...>: capacity 4 * g * v votes per cell; the shapes the dispatch uses:
// (16, 1) (8, 3) (16, 2) (16, 4) (32, 4) (64, 4)
RegKernel pick_reg_kernel(int g, int v, bool tok, bool vec);
RegKernel pick_reg_g8(int v, bool tok, bool vec);      // (8, 3): 65 ... 96 votes in 96 slots, 8-bit bins; (8, 4): an A/B shape for 97 ... 128
RegKernel pick_reg_g16(int v, bool tok, bool vec);
RegKernel pick_reg_g32(int v, bool tok, bool vec);
RegKernel pick_reg_g64(int v, bool tok, bool vec);

// scv_reg_dense<v vectors per lane per part, h parts>: capacity 256 * v * h votes per cell
RegKernel pick_dense_kernel(int v, int h, bool tok, bool vec);

// scv_sort_cells<nv votes per lane>: one lane per cell, 4 <= N <= nv, rows staged by LDS-DMA (scvote_sort.hip.h);
// .waves = the launch bound in waves
RegKernel pick_sort_kernel(int nv, bool tok, bool lin);

// scv_prefix_pool<g lanes per problem, v vectors per lane>: prefix budgets over one pool row per problem, every budget out of one pass
// (scvote_prefix.hip.h); shapes (16, 4) and (32, 4); .waves = the launch bound in waves; words of LDS per wave = prefix_pool_hist_words(g) +
// kPrefixPoolLaneWords; behind the waves ord[B] | nvs[B] | kPrefixPoolFixedWords (the head map) | the counter tables
constexpr int kPrefixPoolLaneWords = 64;          // behind a wave's histograms: one trash word per lane
constexpr int kPrefixPoolFixedWords = 32;
#ifndef SCV_PREFIX_H16
#define SCV_PREFIX_H16 1
#endif
constexpr bool prefix_pool_h16(int g) { return SCV_PREFIX_H16 != 0 && g == 16; }           // 16-bit bins, two per word
constexpr int prefix_pool_hist_words(int g) { return (64 / g) * (prefix_pool_h16(g) ? kBins / 2 : kBins); }
RegKernel pick_prefix_pool_kernel(int g, bool tok, bool vec);

// scv_sort_prefix<nv votes per lane>: prefix budgets that are powers of two (and the whole row) over pools of nv / 2 < N <= nv votes, out of
// one sort per problem (scvote_sort_prefix.hip.h); .waves = the launch bound in waves; LDS words behind the waves' regions:
// sort_prefix_tail_words(nv, B)
constexpr int sort_prefix_classes(int nv) { int l = 0; while ((1 << l) < nv / 2) ++l; return l + 3; }
constexpr long long sort_prefix_tail_words(int nv, int B) { return 16 + ((B + 3) & ~3) + ((sort_prefix_classes(nv) * (nv + 1) + 1) & ~1) + 4 * sort_prefix_classes(nv); }
RegKernel pick_sort_prefix_kernel(int nv, bool tok);

// scv_resample_prefix<tok>: expected majority vote over random orderings of one pool per problem (scv_resample_prefix_i32,
// scvote_resample.hip.h).  One lane per (problem, resample), lanes problem-major, a power-of-two workgroup of 64 / 128 / 256 lanes.
struct ResampleArgs {
    const int32_t* pool; const int32_t* tokens; const int32_t* n_valid; const int32_t* truth;
    int64_t P; int64_t p_offset; uint64_t seed;
    int32_t N, B, R, r_begin, M, np_max;                 // np_max: problem rows a workgroup's chunk of lanes can touch
    unsigned long long* tie_hits; unsigned long long* token_sum; unsigned long long* truth_sum; unsigned long long* per_resample;
    uint32_t* err_flag;
    // appended for the exact form (scv_expected_majority_i32, scvote_expected.hip.h); mode 0 is the shuffle above
    int32_t mode;
    const double* tab;                                   // kExpectedTabWords doubles of the context: binomials | Gauss-Legendre nodes
    double* score_out; double* hit_out;                  // [P, B]; hit_out may be NULL
    // appended for the token-budget vote (scv_token_budget_prefix_i32, scvote_budget.hip.h): n_valid is unused, tokens are required
    const int64_t* budgets;                              // [B] token budgets, any order
    int32_t order;                                       // kOrderPool (x = i, R = 1) | kOrderShuffled (the shuffle above)
    unsigned long long* vote_sum;                        // [B] votes in the prefixes (NULL ok)
    scv_cell* cells_out; int64_t* cell_tokens_out;       // [P, B] (NULL ok; pool order only), overwritten
    // appended for the weighted vote (scv_weighted_prefix_i32, scvote_weighted.hip.h): n_valid holds the budgets, tokens may be NULL
    const int32_t* weights;                              // [P, N] in 0 .. SCV_WEIGHT_MAX
    int32_t rule;                                        // 0: W(v) = sum of the weights (SCV_RULE_WEIGHT_SUM) | 1: their maximum (SCV_RULE_BEST_OF)
    int32_t wlds;                                        // rows staged in LDS as code | weight << 8 words (weighted_rows_in_lds)
    // appended for the adaptive vote (scv_adaptive_prefix_i32, scvote_adaptive.hip.h): n_valid and budgets are unused, tokens may be NULL
    const int32_t* cap; const int32_t* need;             // [B] sample caps | [B, N + 1] stopping table: stop when c1 >= need[b][c2]
    const int32_t* rule_flags;                           // [B] (NULL: all 0) bit 0: SCV_STOP_DECIDED
    unsigned long long* stop_hist;                       // [B, N + 1] cells that stopped after n samples (NULL ok)
    int32_t* cell_votes_out;                             // [P, B] (NULL ok; pool order only), overwritten
    // the vote over draws with replacement (scv_iid_prefix_i32, scvote_iid.hip.h) adds no field: n_valid holds the draw budgets (not clamped
    // to N), tokens may be NULL
    // appended for SCV_FLAG_OPEN_DOMAIN (every body): rows are encoded by resample_encode_row_open, min_mode is a code (scvote_resample.hip.h)
    int32_t open_domain;
    // appended for short-m@k (scv_shortest_prefix_i32, scvote_shortest.hip.h): n_valid holds k_b, tokens are required, token_sum takes the voted tokens
    const int32_t* m_keep;                               // [B] samples kept of the first k_b
    unsigned long long* spent_sum; unsigned long long* latency_sum;     // [B] (NULL ok)
};
using ResampleFn = void (*)(const ResampleArgs);
constexpr int32_t kResampleModeShuffle = 0, kResampleModeExpected = 1, kResampleModeTokenBudget = 2, kResampleModeWeighted = 3,
                  kResampleModeAdaptive = 4, kResampleModeIid = 5, kResampleModeShortest = 6, kResampleModeWide = 7, kResampleModeWideBudget = 8;
constexpr int32_t kOrderPool = 0, kOrderShuffled = 1;    // SCV_ORDER_POOL / SCV_ORDER_SHUFFLED (include/scvote.h)
// LDS words of a token-budget workgroup (scvote_budget.hip.h, in this order): sorted budgets (32 int64) | per-budget sums (3 B int64) |
// budget order [32] | tie classes [B][N + 1] | per-wave encoding scratch (64 each) | per-row truth code and distinct count [np_max][2] |
// the rows as byte codes [np_max][N4] | the lanes' counts [N4][lanes] | their Fisher-Yates arrays [N4][lanes] (shuffled order only)
constexpr long long token_budget_lds_words(int N, int B, int lanes, int np_max, bool shuffled) {
    return 64 + 6LL * B + 32 + (long long)B * (N + 1) + 64LL * (lanes / 64) + 2LL * np_max + (long long)np_max * ((N + 3) / 4) +
           (shuffled ? 2LL : 1LL) * lanes * ((N + 3) / 4);
}
// LDS words of a short-m@k workgroup (scvote_shortest.hip.h, in this order): per-budget sums (4 B int64) | tie classes [B][N + 1] | sorted k_b,
// m_b and their order (3 x 32) | per-wave encoding scratch (64 each) | per-row truth code and distinct count [np_max][2] | the rows as byte
// codes, token ranks and their inverse [np_max][3][N4] | the lanes' counts [N4][lanes] | their rank bitmaps [ceil(N / 32)][lanes] | their
// Fisher-Yates arrays [N4][lanes] (shuffled order only)
constexpr long long shortest_lds_words(int N, int B, int lanes, int np_max, bool shuffled) {
    return 8LL * B + (long long)B * (N + 1) + 96 + 64LL * (lanes / 64) + 2LL * np_max + 3LL * np_max * ((N + 3) / 4) +
           (long long)lanes * ((N + 3) / 4 + (N + 31) / 32) + (shuffled ? (long long)lanes * ((N + 3) / 4) : 0LL);
}
// LDS words of an adaptive-vote workgroup (scvote_adaptive.hip.h, in this order): per-rule sums (3 B int64) | caps [32] | rule masks [2] |
// tie classes [B][N + 1] | stop lengths [B][N + 1] | need as uint16 [B][N + 1] | per-wave encoding scratch (64 each) | per-row truth code and
// distinct count [np_max][2] | the rows as byte codes [np_max][N4] | the lanes' counts [N4][lanes] | their Fisher-Yates arrays (shuffled only)
constexpr long long adaptive_lds_words(int N, int B, int lanes, int np_max, bool shuffled) {
    return 6LL * B + 32 + 2 + 2LL * B * (N + 1) + ((long long)B * (N + 1) + 1) / 2 + 64LL * (lanes / 64) + 2LL * np_max +
           (long long)np_max * ((N + 3) / 4) + (shuffled ? 2LL : 1LL) * lanes * ((N + 3) / 4);
}
// LDS words of a workgroup of the vote over draws with replacement (scvote_iid.hip.h, in this order): per-budget sums (2 B int64) | tie classes
// [B][N + 1] | sorted budgets and their order (2 x 32) | per-wave encoding scratch (64 each) | per-row truth code and distinct count [np_max][2] |
// the rows as byte codes [np_max][N4] | the lanes' 16-bit counts, two per word [(N + 1) / 2][lanes]
constexpr long long iid_lds_words(int N, int B, int lanes, int np_max) {
    return 4LL * B + (long long)B * (N + 1) + 64 + 64LL * (lanes / 64) + 2LL * np_max + (long long)np_max * ((N + 3) / 4) + (long long)lanes * ((N + 1) / 2);
}
// The weighted body stages a row as N words (code | weight << 8) when a chunk of lanes touches few rows, R >= kWeightedLdsRowsMinR (at most
// lanes / R + 2 rows); below that -- and in pool order, R = 1 -- as byte codes, with the weight read from global memory: lanes + 1 rows of N words
// would not fit beside the lanes' totals.
constexpr int kWeightedLdsRowsMinR = 64;
constexpr bool weighted_rows_in_lds(long long R, bool shuffled) { return shuffled && R >= kWeightedLdsRowsMinR; }
// LDS words of a weighted-vote workgroup (scvote_weighted.hip.h, in this order): per-budget token sums (B int64) | tie classes [B][N + 1] |
// sorted budgets and their order (2 x 32) | per-wave encoding scratch (64 each) | per-row truth code and distinct count [np_max][2] | the rows
// [np_max][N words or N4 words of byte codes] | the lanes' uint32 totals [N][lanes] | their Fisher-Yates arrays [N4][lanes] (shuffled order only)
constexpr long long weighted_lds_words(int N, int B, int lanes, int np_max, bool shuffled, bool wlds) {
    return 2LL * B + (long long)B * (N + 1) + 64 + 64LL * (lanes / 64) + 2LL * np_max + (long long)np_max * (wlds ? N : (N + 3) / 4) +
           (long long)lanes * N + (shuffled ? (long long)lanes * ((N + 3) / 4) : 0LL);
}
// the context's table (kExpectedTabWords doubles: binomials | Gauss-Legendre rules) and its layout: scvote_expected_table.h
constexpr int kExpectedLanes = 256;
constexpr int kExpectedVec = 256 + 8;                     // 256 coefficients, one pad double per 32
constexpr int kExpectedZeros = 136;                       // zeros in front: the slots of coefficients -129 .. -1 (a factor's degree is <= 128)
// LDS bytes of a workgroup of `lanes` lanes: vectors [waves][kExpectedZeros + kExpectedVec] | E and H sums [2][waves][32] (doubles), then the int32 words:
// votes per code [256] | classes per count [260] (hist[257]: the largest count) | meta [4] | the row's codes [64] | encoding scratch [64]
constexpr long long expected_lds_bytes(int lanes) { return 8LL * ((lanes / 64) * (kExpectedZeros + kExpectedVec) + 2 * (lanes / 64) * 32) + 4LL * (256 + 260 + 4 + 64 + 64); }
constexpr int kResampleMaxN = 256, kResampleMaxB = 32, kResampleMaxLanes = 256;
// LDS words of a workgroup of `lanes` lanes (the kernel's layout, in this order): per-budget sums (2 B int64) | tie classes [B][N + 1] |
// sorted budgets and their order (2 x 32) | per-wave encoding scratch (64 each) | per-row truth code and distinct count [np_max][2] |
// the rows as byte codes [np_max][N4] | the lanes' Fisher-Yates arrays [N4][lanes] | their counts [N4][lanes]
constexpr long long resample_lds_words(int N, int B, int lanes, int np_max) {
    return 4LL * B + (long long)B * (N + 1) + 64 + 64LL * (lanes / 64) + 2LL * np_max + (long long)np_max * ((N + 3) / 4) + 2LL * lanes * ((N + 3) / 4);
}
// The wide body (scv_resample_wide_i32, scvote_wide.hip.h; mode kResampleModeWide of the <false> instantiation): one workgroup per (problem,
// resample), 1 <= N <= SCV_WIDE_MAX_N.  The sort runs over wide_pad(N) words (the next power of two, at least 2); the workgroup has one lane per
// compare-exchange of a stage, 64 .. 256; the LDS tie table has wide_tie_cols(N) columns, larger classes go to global memory one by one.
constexpr int wide_pad(int N) { int n2 = 2; while (n2 < N) n2 <<= 1; return n2; }
constexpr int wide_lanes(int N) { const int h = wide_pad(N) / 2; return h < 64 ? 64 : (h > kResampleMaxLanes ? kResampleMaxLanes : h); }
constexpr int wide_tie_cols(int N) { return (N < 127 ? N : 127) + 1; }
// LDS words of a wide workgroup (the kernel's layout, in this order): the sort words (wide_pad(N) uint64) | per-budget sums (2 B int64) | the
// waves' token sums (2 x 4 int64) | the histogram (wide_hist_words) | tie classes [B][wide_tie_cols(N)] | the waves' (max, modes) (2 x 4 x 2) |
// sorted budgets and their order (2 x 32) | the row as 16-bit bins [N]
// The histogram: 1024 words, one per bin; under SCV_FLAG_OPEN_DOMAIN max(1024, N) 16-bit counts, two per word (a row has at most N distinct
// values and a count is at most N <= 4096).
constexpr long long wide_hist_words(int N, bool open) { return open ? ((N > kBins ? N : kBins) + 1) / 2 : kBins; }
constexpr long long wide_lds_words(int N, int B, bool open) {
    return 2LL * wide_pad(N) + 4LL * B + 16 + wide_hist_words(N, open) + (long long)B * wide_tie_cols(N) + 16 + 64 + (N + 1) / 2;
}
// LDS words of a wide token-budget workgroup (scv_token_budget_wide_i32, scvote_wide_budget.hip.h; mode kResampleModeWideBudget of the <false>
// instantiation; the kernel's layout, in this order): the sort words, later running sum << 12 | index (wide_pad(N) uint64) | per-budget sums
// (3 B int64: truth counts, tokens, votes) | sorted budgets (32 int64) | the waves' token sums of the scan (4 int64) | the histogram
// (wide_hist_words) | tie classes [B][wide_tie_cols(N)] | the waves' (largest count << 12 | 4095 - its smallest bin, modes) (2 x 4 x 2) | the item's prefix lengths and
// the budgets' order (2 x 32) | the row as 16-bit bins [N].  224 + 8 B bytes more than wide_lds_words.
constexpr long long wide_budget_lds_words(int N, int B, bool open) {
    return 2LL * wide_pad(N) + 6LL * B + 64 + 8 + wide_hist_words(N, open) + (long long)B * wide_tie_cols(N) + 16 + 64 + (N + 1) / 2;
}
ResampleFn pick_resample_kernel(bool tok);

// ---- shared by the table translation units ------------------------------------------------------------------------
template <int RL2, int T, int U>
inline KernelFn stream_tok(bool tok, bool xtra) {
    if (xtra) return tok ? (KernelFn)scv_hist_argmax<RL2, T, U, true, true> : (KernelFn)scv_hist_argmax<RL2, T, U, false, true>;
    return tok ? (KernelFn)scv_hist_argmax<RL2, T, U, true> : (KernelFn)scv_hist_argmax<RL2, T, U, false>;
}
template <int RL2, int T, int U>
inline KernelFn stream_plain(bool tok) {
    return tok ? (KernelFn)scv_hist_argmax<RL2, T, U, true> : (KernelFn)scv_hist_argmax<RL2, T, U, false>;
}
template <int G, int V, int K>
inline RegKernel reg_gv(bool tok, bool vec) {
    if (tok) return vec ? RegKernel{(KernelFn)scv_reg_cells<G, V, K, true, true>, reg_cells_waves<G, V, true, true>()}
                        : RegKernel{(KernelFn)scv_reg_cells<G, V, K, true, false>, reg_cells_waves<G, V, true, false>()};
    return vec ? RegKernel{(KernelFn)scv_reg_cells<G, V, K, false, true>, reg_cells_waves<G, V, false, true>()}
               : RegKernel{(KernelFn)scv_reg_cells<G, V, K, false, false>, reg_cells_waves<G, V, false, false>()};
}

}  // namespace scv
