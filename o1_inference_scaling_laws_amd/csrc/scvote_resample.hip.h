// scvote_resample.hip.h -- expected majority vote over random orderings of one sample pool per problem (scv_resample_prefix<TOK>).
//
// The reference's budgets T >= 2^11 vote over the FIRST N_b samples of one pool (o1.py:274-277 with the idx-keyed cache of
// o1.py:85-88): every point of that curve is one draw.  scv_resample_prefix_i32 (include/scvote.h) draws R orderings per problem
// by a counter-based partial Fisher-Yates shuffle and votes over the prefixes of each: sum over orderings of the tie-class hits is
// P * R times the expected maj@k.  The work is P * R * max_b k_b shuffle steps over a pool read once: VALU / LDS-bound, not HBM-bound.
//
// How:
//  * one lane per (problem, resample), flattened problem-major, so a wave touches one or two problems when R >= 64.  A persistent
//    workgroup walks chunks of `lanes` consecutive (problem, resample) pairs.
//  * per chunk, every problem row the chunk touches is re-encoded ONCE into LDS by one wave: a 1024-bit presence map of the votes
//    (votes outside 0..1023 go to bin 1023 and raise error bit 0), its running popcount, and from them every vote's rank among the
//    row's distinct values -- a dense code < N (<= 256, one byte) -- and the truth's code, or -1 when the truth is not in the row or
//    not in the bins (it never hits).
//  * every lane owns two byte arrays of ceil(N / 4) words in LDS, laid out [slot / 4][lane]: the Fisher-Yates array and the counts over
//    the row's codes.  Byte e of lane l lives in word (e / 4) * lanes + l, so the 32 lanes of an access group always hit 32 different
//    banks, whatever slot each lane picked.  Without tokens the shuffled array holds the CODES themselves (one LDS read less per
//    step); with tokens it holds pool indices (0..255), the code is looked up in the row and the token read from global memory (the
//    row is a few hundred bytes that every lane of the problem reads: L1 / L2 hits).
//  * step i: u = mix64(arg), arg += G; j = i + mulhi32(hi32(u), N - i); x = a[j]; a[j] = a[i] (slot i is never read again);
//    c = ++cnt[code].  Counts only grow by one, so the mode statistics are kept running: c > max -> (max, n_modes) = (c, 1);
//    c == max -> n_modes + 1.  Byte counts are exact: a count of 256 needs 256 votes of one value -- only at the very last step of
//    N = 256, and that count is never read back.  The truth's count is a register (tc += code == truth code): hit = tc == max > 0.
//  * budgets are sorted once per workgroup (rank sort in LDS) and are the same for every lane, so the boundary test is uniform; at
//    a boundary the wave adds its lanes' hits to the workgroup's LDS tables (one ballot for the common n_modes == 1, an LDS atomic
//    for the rest), its truth-count and token sums (DPP reductions), and -- when requested -- each hit to per_resample with one
//    global atomic (lanes of a wave hold different resamples).  The tables are flushed with non-returning int64 atomics once per
//    workgroup (the 32-bit tie table also every floor((2^32 - 1) / lanes) chunks of it, so that no counter wraps).  No scratch buffer,
//    no allocation: a DEVICE-mode call is one launch and may be captured into a graph.
//
// LDS per lane 2 * 4 * ceil(N / 4) bytes (N = 128: 16 KiB per wave, 10 waves per CU of 160 KiB; N = 256: 32 KiB per wave, 5 waves).
// The <false> instantiation has five more bodies: the exact form of the same expectation (mode kResampleModeExpected, scvote_expected.hip.h),
// the weighted vote / best-of-N (mode kResampleModeWeighted, scvote_weighted.hip.h), the vote over draws with replacement (mode
// kResampleModeIid, scvote_iid.hip.h), the sorted orderings of pools of up to 4096 samples (mode kResampleModeWide, scvote_wide.hip.h,
// workgroup-cooperative like the exact form) and the token budgets over those orderings (mode kResampleModeWideBudget,
// scvote_wide_budget.hip.h); the <true> one the vote over the longest prefix
// that fits a token budget (mode kResampleModeTokenBudget, scvote_budget.hip.h), the vote that stops by a rule on its own state
// (mode kResampleModeAdaptive, scvote_adaptive.hip.h) and the vote over the m shortest of the first k samples (mode kResampleModeShortest,
// scvote_shortest.hip.h).
#pragma once

#include "scvote_kernels.hip.h"
#include "scvote_dispatch.h"

namespace scv {

constexpr uint64_t kResampleSalt = 0xD6E8FEB86659FD93ull;

// byte e of a lane's [slot / 4][lane] array: word (e >> 2) * lanes + lane
__device__ __forceinline__ uint32_t resample_byte(uint32_t e, int lanes_log2, uint32_t lane_byte) {
    return ((e >> 2) << (lanes_log2 + 2)) + (e & 3u) + lane_byte;
}

// One wave turns up to 256 votes that lie in 0..1023 (v[k]: element lane + 64 k) into value-ordered byte codes: a 1024-bit presence map, its running
// popcount and from them every vote's rank among the row's distinct values.  meta[0] = the code of t = truth_of() (evaluated by lane 0 only), or -1
// when t is outside the bins or not in the row; meta[1] = the number of distinct values.  scr: 64 words of the wave's own.
template <class TruthOf>
__device__ __forceinline__ void resample_encode_binned(const int32_t (&v)[kResampleMaxN / 64], TruthOf truth_of, int N, uint8_t* row_codes, int32_t* meta,
                                                       uint32_t* scr, int lane) {
    if (lane < 32) scr[lane] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        const int32_t x = v[k];
        if (e < N) atomicOr(&scr[x >> 5], 1u << (x & 31));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // exclusive popcount prefix of the 32 map words (lanes 0..31), total in lane 31's inclusive value
    const uint32_t word = lane < 32 ? scr[lane] : 0u;
    uint32_t incl = (uint32_t)__popc(word);
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)incl, d, 64);
        if ((lane & 31) >= d) incl += u;
    }
    if (lane < 32) scr[32 + lane] = incl - (uint32_t)__popc(word);
    const int32_t distinct = __shfl((int)incl, 31, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        if (e < N) {
            const uint32_t x = (uint32_t)v[k];
            row_codes[e] = (uint8_t)(scr[32 + (x >> 5)] + (uint32_t)__popc(scr[x >> 5] & ((1u << (x & 31)) - 1u)));
        }
    }
    if (lane == 0) {
        const int32_t t = truth_of();
        int32_t tcode = -1;
        if ((uint32_t)t < (uint32_t)kBins && ((scr[t >> 5] >> (t & 31)) & 1u))
            tcode = (int32_t)(scr[32 + (t >> 5)] + (uint32_t)__popc(scr[t >> 5] & ((1u << (t & 31)) - 1u)));
        meta[0] = tcode;
        meta[1] = distinct;
    }
}

// one wave re-encodes the pool row of problem p into value-ordered byte codes: row_codes (bytes), meta[0] = the truth's code or -1,
// meta[1] = the number of distinct values.  scr: 64 words of the wave's own.  Returns true when a vote was outside 0..1023.
__device__ __forceinline__ bool resample_encode_row(const ResampleArgs& a, int64_t p, uint8_t* row_codes, int32_t* meta, uint32_t* scr, int lane) {
    const int N = a.N;
    const int32_t* row = a.pool + p * (int64_t)N;
    int32_t v[kResampleMaxN / 64];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        int32_t x = e < N ? row[e] : 0;
        if ((uint32_t)x >= (uint32_t)kBins) { bad = bad || e < N; x = kBins - 1; }
        v[k] = x;
    }
    resample_encode_binned(v, [&] { return a.truth[p]; }, N, row_codes, meta, scr, lane);
    return bad;
}

// The same contract for SCV_FLAG_OPEN_DOMAIN: every int32 is a value of its own, ordered as signed integers; never a domain error (returns false).
// Rank by counting, in registers: element j is broadcast from its lane (a readlane into a scalar register; j and N are uniform) and every lane
// counts it against its own four keys, so after N steps lt[k] is the number of votes BELOW key k.  Equal keys have equal counts, a larger key a
// larger one (it is above every vote the smaller key is above, and above that key itself), and every count is below N <= 256: the counts are an
// order-preserving relabelling of the row INTO the bins, and the binned encoder makes them dense.  The truth takes the count of the vote it equals.
// Per broadcast step, read from the gfx950 ISA: one v_readlane_b32 and, per register that holds votes, one v_cmp_lt_i32 and one add (a
// v_addc_co_u32 that takes one compare as its carry and a second through a v_cndmask_b32): 3 / 5.1-5.3 / 7-7.8 / 9-10 VALU for 1 / 2 / 3 / 4
// registers (192 per row at N = 64, ~660 at 128, ~2400 at 256).  No LDS beyond the binned encoder's 64 words.
// one broadcast step: key j of register src goes to a scalar register, every lane counts it against its NK keys
template <int NK>
__device__ __forceinline__ void open_count_step(int32_t src, int jl, const int32_t (&key)[kResampleMaxN / 64], int32_t (&lt)[kResampleMaxN / 64]) {
    const int32_t s = __builtin_amdgcn_readlane(src, jl);
#pragma unroll
    for (int k = 0; k < NK; ++k) lt[k] += s < key[k] ? 1 : 0;
}
// lt[k] += votes below key[k], for the NK registers of a row of N votes, 64 (NK - 1) < N <= 64 NK.  Full registers take the loop of constant length,
// which the compiler unrolls (the last one too when N = 64 NK: 64, 128, 192, 256); only a ragged last register takes the rolled one.
template <int NK>
__device__ __forceinline__ void open_count_below(const int32_t (&key)[kResampleMaxN / 64], int32_t (&lt)[kResampleMaxN / 64], int N) {
    const int tail = N - 64 * (NK - 1);
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
        if (kk < NK - 1 || tail == 64) {
            for (int jl = 0; jl < 64; ++jl) open_count_step<NK>(key[kk], jl, key, lt);
        } else {
            for (int jl = 0; jl < tail; ++jl) open_count_step<NK>(key[kk], jl, key, lt);
        }
    }
}

// Outlined, with its three LDS pointers as 32-bit LDS addresses: the bodies keep their register counts, and a flag-off launch never enters it.
using lds_u8 = __attribute__((address_space(3))) uint8_t;
using lds_i32 = __attribute__((address_space(3))) int32_t;
using lds_u32 = __attribute__((address_space(3))) uint32_t;
__device__ __noinline__ void resample_encode_row_open(const int32_t* row, int32_t t, int N_arg, lds_u8* row_codes_l, lds_i32* meta_l, lds_u32* scr_l) {
    const int N = __builtin_amdgcn_readfirstlane(N_arg);                            // arguments of a real call arrive in VGPRs: N is uniform, say so
    const int lane = (int)threadIdx.x & 63;
    uint8_t* row_codes = (uint8_t*)row_codes_l;
    int32_t* meta = (int32_t*)meta_l;
    uint32_t* scr = (uint32_t*)scr_l;
    int32_t key[kResampleMaxN / 64], lt[kResampleMaxN / 64];
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        key[k] = e < N ? row[e] : 0;
        lt[k] = 0;
    }
    const int nk = (N + 63) >> 6;                                                    // registers that hold a vote (scalar, like N)
    if (nk == 1) open_count_below<1>(key, lt, N);
    else if (nk == 2) open_count_below<2>(key, lt, N);
    else if (nk == 3) open_count_below<3>(key, lt, N);
    else open_count_below<4>(key, lt, N);
    int32_t mine = -1;
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k)
        if (lane + 64 * k < N && key[k] == t) mine = lt[k];
    const unsigned long long has = __ballot(mine >= 0);
    const int32_t tl = has ? __shfl(mine, __ffsll(has) - 1, 64) : -1;
    resample_encode_binned(lt, [&] { return tl; }, N, row_codes, meta, scr, lane);
}

// the encoder of a context: open_domain is uniform over the launch
__device__ __forceinline__ bool resample_encode(const ResampleArgs& a, int64_t p, uint8_t* row_codes, int32_t* meta, uint32_t* scr, int lane) {
    if (a.open_domain) { resample_encode_row_open(a.pool + p * (int64_t)a.N, a.truth[p], a.N, (lds_u8*)row_codes, (lds_i32*)meta, (lds_u32*)scr); return false; }
    return resample_encode_row(a, p, row_codes, meta, scr, lane);
}

// min_mode of a pool-order cell (token-budget, weighted, adaptive bodies): x is a sample of the smallest modal value, code its byte code.  The
// value itself, clamped into the bins; under SCV_FLAG_OPEN_DOMAIN the code (an int16 cannot hold an arbitrary int32).
__device__ __forceinline__ int32_t resample_min_mode(const ResampleArgs& a, int64_t p, uint32_t x, uint32_t code) {
    if (a.open_domain) return (int32_t)code;
    int32_t mm = a.pool[p * (int64_t)a.N + x];
    if ((uint32_t)mm >= (uint32_t)kBins) mm = kBins - 1;
    return mm;
}

}  // namespace scv

#include "scvote_expected.hip.h"
#include "scvote_budget.hip.h"
#include "scvote_weighted.hip.h"
#include "scvote_adaptive.hip.h"
#include "scvote_shortest.hip.h"
#include "scvote_iid.hip.h"
#include "scvote_wide.hip.h"
#include "scvote_wide_budget.hip.h"

namespace scv {

template <bool TOK>
__global__ __launch_bounds__(kResampleMaxLanes) void scv_resample_prefix(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem_wg[];
    if constexpr (!TOK) {
        if (a.mode == kResampleModeExpected) { expected_majority_body(a, smem_wg); return; }    // the exact form: scvote_expected.hip.h
        if (a.mode == kResampleModeWeighted) { weighted_body(a, smem_wg); return; }             // weighted vote / best-of-N: scvote_weighted.hip.h
        if (a.mode == kResampleModeIid) { iid_body(a, smem_wg); return; }                       // draws with replacement: scvote_iid.hip.h
        if (a.mode == kResampleModeWide) { wide_body(a, smem_wg); return; }                     // pools of up to 4096 samples: scvote_wide.hip.h
        if (a.mode == kResampleModeWideBudget) { wide_budget_body(a, smem_wg); return; }        // ... under token budgets: scvote_wide_budget.hip.h
    } else {
        if (a.mode == kResampleModeTokenBudget) { token_budget_body(a, smem_wg); return; }      // token budgets: scvote_budget.hip.h
        if (a.mode == kResampleModeAdaptive) { adaptive_body(a, smem_wg); return; }             // stopping rules: scvote_adaptive.hip.h
        if (a.mode == kResampleModeShortest) { shortest_body(a, smem_wg); return; }             // short-m@k: scvote_shortest.hip.h
    }
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int lanes_log2 = 31 - __clz(lanes);
    const int N = a.N, B = a.B, N4 = (N + 3) >> 2, TC = N + 1;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem_wg);      // [B] truth-count sums | [B] token sums
    uint32_t* tie = smem_wg + 4 * B;                                                // [B][N + 1]
    int32_t* ks = reinterpret_cast<int32_t*>(tie + B * TC);                         // [32] budgets, ascending
    int32_t* ord = ks + 32;                                                         // [32] their indices
    uint32_t* scr = reinterpret_cast<uint32_t*>(ord + 32);                          // [nwaves][64]
    int32_t* meta = reinterpret_cast<int32_t*>(scr + 64 * nwaves);                  // [np_max][2]
    uint32_t* rows = reinterpret_cast<uint32_t*>(meta + 2 * a.np_max);              // [np_max][N4]
    uint32_t* arr = rows + a.np_max * N4;                                           // [N4][lanes]
    uint32_t* cnt = arr + N4 * lanes;                                               // [N4][lanes]
    uint8_t* arr_b = reinterpret_cast<uint8_t*>(arr);
    uint8_t* cnt_b = reinterpret_cast<uint8_t*>(cnt);
    const uint8_t* rows_b = reinterpret_cast<const uint8_t*>(rows);

    for (int i = tid; i < B * TC; i += lanes) tie[i] = 0u;
    if (tid < 2 * B) acc[tid] = 0ull;
    if (tid < B) {                                                                  // rank sort: ties keep index order
        int32_t k = a.n_valid[tid];
        k = k < 0 ? 0 : (k > N ? N : k);
        int rank = 0;
        for (int b = 0; b < B; ++b) {
            int32_t kb = a.n_valid[b];
            kb = kb < 0 ? 0 : (kb > N ? N : kb);
            rank += (kb < k || (kb == k && b < tid)) ? 1 : 0;
        }
        ks[rank] = k;
        ord[rank] = tid;
    }
    __syncthreads();
    const int32_t kmax = ks[B - 1];
    int q0 = 0;
    while (q0 < B && ks[q0] == 0) ++q0;                                              // empty subsets: no hit, nothing to add
    const int64_t R = a.R, total = a.P * R;
    const int64_t nchunks = (total + lanes - 1) / lanes;
    const uint32_t lane_byte = (uint32_t)tid << 2;
    bool bad = false, overflow = false;
    // A chunk adds at most `lanes` to one tie counter (one per lane and budget), and P * R may reach 2^62 with one workgroup doing all:
    // the workgroup's chunks go in epochs of floor((2^32 - 1) / lanes), and the 32-bit table is flushed into the int64 outputs between
    // two epochs, before any counter can wrap.
    const int64_t epoch = (int64_t)(0xffffffffu / (uint32_t)lanes) * gridDim.x;
    for (int64_t c0 = blockIdx.x; c0 < nchunks; c0 += epoch) {
    const int64_t c1 = nchunks - c0 > epoch ? c0 + epoch : nchunks;
    for (int64_t chunk = c0; chunk < c1; chunk += gridDim.x) {
        const int64_t t0 = chunk * lanes;
        const int64_t p_lo = t0 / R;
        int64_t p_hi = (t0 + lanes - 1) / R;
        if (p_hi > a.P - 1) p_hi = a.P - 1;
        for (int64_t pl = wave; pl <= p_hi - p_lo; pl += nwaves)
            bad |= resample_encode(a, p_lo + pl, reinterpret_cast<uint8_t*>(rows + pl * N4), meta + 2 * pl, scr + 64 * wave, lane);
        __syncthreads();
        const int64_t t = t0 + tid;
        const bool live = t < total;
        const int64_t p = (live ? t : total - 1) / R;
        const int32_t rr = (int32_t)((live ? t : total - 1) - p * R);
        const int32_t row = (int32_t)(p - p_lo);
        const int32_t tcode = meta[2 * row], distinct = meta[2 * row + 1];
        for (int w = 0; w < N4; ++w) arr[(w << lanes_log2) + tid] = TOK ? 0x03020100u + 0x04040404u * (uint32_t)w : rows[row * N4 + w];
        for (int w = 0; w < ((distinct + 3) >> 2); ++w) cnt[(w << lanes_log2) + tid] = 0u;
        const uint8_t* my_row = rows_b + (int64_t)row * N4 * 4;
        const int32_t* tok_row = TOK ? a.tokens + p * (int64_t)N : nullptr;
        const uint64_t s = mix64((a.seed ^ kResampleSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
        uint64_t arg = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)N + 1ull);
        uint32_t maxc = 0, nmodes = 0, tc = 0;
        long long tok = 0;
        int q = q0;
        int32_t next_k = q < B ? ks[q] : 0x7fffffff;
        for (int32_t i = 0; i < kmax; ++i) {
            const uint64_t u = mix64(arg);
            arg += kGolden;
            const uint32_t j = (uint32_t)i + mulhi32((uint32_t)(u >> 32), (uint32_t)(N - i));
            const uint32_t ai = arr_b[resample_byte((uint32_t)i, lanes_log2, lane_byte)];
            const uint32_t aj = resample_byte(j, lanes_log2, lane_byte);
            const uint32_t x = arr_b[aj];
            arr_b[aj] = (uint8_t)ai;
            const uint32_t code = TOK ? (uint32_t)my_row[x] : x;
            const uint32_t ac = resample_byte(code, lanes_log2, lane_byte);
            const uint32_t c = (uint32_t)cnt_b[ac] + 1u;
            cnt_b[ac] = (uint8_t)c;
            if (c > maxc) { maxc = c; nmodes = 1u; }
            else if (c == maxc) nmodes += 1u;
            tc += (int32_t)code == tcode ? 1u : 0u;
            if (TOK) tok += tok_row[x];
            if (i + 1 == next_k) {
                const bool hit = live && tcode >= 0 && tc == maxc;
                const uint32_t tcs = wave_sum_u32(live ? tc : 0u);
                const long long toks = TOK ? wave_sum_i64(live ? tok : 0ll) : 0ll;
                const unsigned long long ones = __ballot(hit && nmodes == 1u);
                do {                                                                  // every budget of this size
                    const int32_t b = ord[q];
                    if (lane == 0) {
                        if (ones) atomicAdd(&tie[b * TC + 1], (uint32_t)__popcll(ones));
                        if (tcs) atomicAdd(&acc[b], (unsigned long long)tcs);
                        if (TOK && toks) atomicAdd(&acc[B + b], (unsigned long long)toks);
                    }
                    if (hit && nmodes != 1u) atomicAdd(&tie[b * TC + nmodes], 1u);
                    if (hit && a.per_resample) {
                        if (nmodes < (uint32_t)a.M) atomicAdd(&a.per_resample[((int64_t)rr * B + b) * a.M + nmodes], 1ull);
                        else overflow = true;
                    }
                    ++q;
                    next_k = q < B ? ks[q] : 0x7fffffff;
                } while (next_k == i + 1);
            }
        }
        __syncthreads();                                                              // the rows are rewritten by the next chunk
    }
    if (c1 < nchunks) {                                                               // another epoch follows (uniform)
        for (int i = tid; i < B * TC; i += lanes) {
            const uint32_t v = tie[i];
            if (v) { atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v); tie[i] = 0u; }
        }
        __syncthreads();
    }
    }
    if (__ballot(bad) && lane == 0) atomicOr(a.err_flag, 1u);
    if (__ballot(overflow) && lane == 0) atomicOr(a.err_flag, 2u);
    __syncthreads();
    for (int i = tid; i < B * TC; i += lanes) {
        const uint32_t v = tie[i];
        if (v) atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v);
    }
    if (tid < B) {
        if (a.truth_sum && acc[tid]) atomicAdd(&a.truth_sum[tid], acc[tid]);
        if (TOK && a.token_sum && acc[B + tid]) atomicAdd(&a.token_sum[tid], acc[B + tid]);
    }
}

}  // namespace scv
