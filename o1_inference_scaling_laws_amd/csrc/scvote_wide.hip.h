// scvote_wide.hip.h -- expected majority vote over random orderings of pools of up to 4096 samples (scv_resample_wide_i32): a further body of
// scv_resample_prefix<false> (mode kResampleModeWide), included by scvote_resample.hip.h.
//
// The lane bodies keep one lane per (problem, ordering) with a byte permutation per lane in LDS: 256 samples at most.  Here a whole workgroup
// owns one (problem, resample) item, and the ordering is not walked but SORTED: w_i = (mix64(s + G (r 4096 + i + 1)) & ~4095) | i, ascending
// (include/scvote.h).  The words are distinct, so any sorting network gives the one order.
//
// How:
//  * persistent grid; a workgroup takes a contiguous run of ceil(P R / grid) items, r innermost: a problem's row is read from global memory
//    once per run and kept in LDS as 16-bit bins (a vote outside 0..1023 goes to bin 1023 and raises error bit 0).
//  * per item the N words are built in LDS, padded with all-ones to n2 = the next power of two, and sorted by a bitonic network: every
//    compare-exchange of a stage is independent, lanes take them round-robin, one workgroup barrier per stage (log2 n2 (log2 n2 + 1) / 2).
//  * the sorted order is walked budget by budget in ascending k_b.  A segment adds its votes into ONE 1024-bin histogram (non-returning LDS
//    atomics) and its tokens -- gathered from global memory by pool index: the row is at most 16 KiB that the R items of a problem share,
//    L1 / L2 hits, and staging it would halve the workgroups per CU at N = 4096 -- into a per-lane running sum.  At a boundary every lane scans
//    1024 / lanes bins for (max count, bins at the max), the waves reduce on the VALU (DPP) and exchange three words through LDS; the truth's
//    count is its bin.  Two barriers per boundary; the exchange slots alternate, so the next segment starts behind the second.
//  * lane 0 emits: the tie class into the workgroup's LDS table when n_modes < the table's columns (min(N, 127) + 1: n_modes is 1 for nearly
//    every cell), else one global atomic; truth-count and token sums into 64-bit LDS tables; per_resample with one global atomic per hit.
//    The tables are flushed with non-returning int64 atomics once per workgroup (the 32-bit tie table also every 2^31 - 1 items, so no
//    counter wraps).  No scratch buffer, no allocation: a DEVICE-mode call is one launch and may be captured into a graph.
//
// LDS words: wide_lds_words (scvote_dispatch.h).  N = 4096, B = 13: 32 KiB of words + 8 KiB of bins + 4 KiB of histogram + 6.6 KiB of tables.
#pragma once

namespace scv {

constexpr uint64_t kWideSalt = 0x8EBC6AF09C88C6E3ull;

__device__ __forceinline__ void wide_body(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int N = a.N, B = a.B;
    const int n2 = wide_pad(N), TCL = wide_tie_cols(N);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);         // [n2] the sort words
    unsigned long long* acc = keys + n2;                                            // [B] truth-count sums | [B] token sums
    unsigned long long* red_tok = acc + 2 * B;                                      // [2][4] the waves' token sums, slots alternate
    uint32_t* hist = reinterpret_cast<uint32_t*>(red_tok + 8);                      // [1024]
    uint32_t* tie = hist + kBins;                                                   // [B][TCL]
    uint32_t* red = tie + B * TCL;                                                  // [2][4][2] the waves' (max count, bins at the max)
    int32_t* ks = reinterpret_cast<int32_t*>(red + 16);                             // [32] budgets, ascending
    int32_t* ord = ks + 32;                                                         // [32] their indices
    uint16_t* bins = reinterpret_cast<uint16_t*>(ord + 32);                         // [N] the row

    for (int i = tid; i < B * TCL; i += lanes) tie[i] = 0u;
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
    int q0 = 0;
    while (q0 < B && __builtin_amdgcn_readfirstlane(ks[q0]) == 0) ++q0;             // empty prefixes: no hit, nothing to add

    auto flush_tie = [&] {
        for (int i = tid; i < B * TCL; i += lanes) {
            const uint32_t v = tie[i];
            if (v) { atomicAdd(&a.tie_hits[(int64_t)(i / TCL) * SCV_TIE_CLASSES + (i % TCL)], (unsigned long long)v); tie[i] = 0u; }
        }
    };

    const int64_t R = a.R, total = a.P * R;
    const int64_t per_wg = (total + gridDim.x - 1) / gridDim.x;
    const int64_t it0 = (int64_t)blockIdx.x * per_wg;
    const int64_t it1 = total - it0 < per_wg ? total : it0 + per_wg;
    int64_t p = it0 < total ? it0 / R : 0;
    int32_t rr = it0 < total ? (int32_t)(it0 - p * R) : 0;
    bool bad = false, fresh = true;
    int32_t tbin = -1;
    uint32_t since_flush = 0;
    for (int64_t it = it0; it < it1; ++it) {
        if (fresh) {                                                                // a new problem: its row, its truth (the last item's reads lie behind two barriers)
            const int32_t* row = a.pool + p * (int64_t)N;
            for (int e = tid; e < N; e += lanes) {
                int32_t x = row[e];
                if ((uint32_t)x >= (uint32_t)kBins) { bad = true; x = kBins - 1; }
                bins[e] = (uint16_t)x;
            }
            const int32_t t = a.truth[p];
            tbin = (uint32_t)t < (uint32_t)kBins ? t : -1;
            fresh = false;
        }
        const uint64_t s = mix64((a.seed ^ kWideSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
        const uint64_t base = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)SCV_WIDE_MAX_N + 1ull);
        for (int i = tid; i < n2; i += lanes)
            keys[i] = i < N ? ((mix64(base + kGolden * (uint64_t)i) & ~(uint64_t)(SCV_WIDE_MAX_N - 1)) | (uint64_t)i) : ~0ull;
        for (int i = tid; i < kBins; i += lanes) hist[i] = 0u;
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1) {                                         // bitonic network over keys[0 .. n2)
            for (int j = k >> 1; j > 0; j >>= 1) {
#pragma nounroll
                for (int t = tid; t < (n2 >> 1); t += lanes) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));           // the pair (lo, lo + j)
                    const unsigned long long x = keys[lo], y = keys[lo + j];
                    if ((x > y) == ((lo & k) == 0)) { keys[lo] = y; keys[lo + j] = x; }
                }
                __syncthreads();
            }
        }
        const int32_t* tok_row = a.tokens ? a.tokens + p * (int64_t)N : nullptr;
        long long tok = 0;
        int32_t at = 0;
        int q = q0, flip = 0;
        while (q < B) {
            const int32_t k = __builtin_amdgcn_readfirstlane(ks[q]);
            for (int32_t e = at + tid; e < k; e += lanes) {
                uint32_t idx = (uint32_t)keys[e] & (uint32_t)(SCV_WIDE_MAX_N - 1);
                idx = idx < (uint32_t)N ? idx : (uint32_t)N - 1u;                    // (the first N sorted words are the samples': idx is a pool index)
                __hip_atomic_fetch_add(&hist[bins[idx]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (tok_row) tok += tok_row[idx];
            }
            at = k;
            __syncthreads();
            uint32_t mx = 0, nm = 0;
#pragma nounroll
            for (int i = tid; i < kBins; i += lanes) {
                const uint32_t c = hist[i];
                if (c > mx) { mx = c; nm = 1u; }
                else if (c == mx) nm += 1u;
            }
            const uint32_t tc = tbin >= 0 ? hist[tbin] : 0u;
            const uint32_t wmx = wave_max_u32(mx);
            const uint32_t wnm = wave_sum_u32(mx == wmx ? nm : 0u);
            const long long wtok = tok_row ? wave_sum_i64(tok) : 0ll;
            if (lane == 0) {
                red[flip * 8 + wave * 2] = wmx;
                red[flip * 8 + wave * 2 + 1] = wnm;
                red_tok[flip * 4 + wave] = (unsigned long long)wtok;
            }
            __syncthreads();
            uint32_t maxc = 0, nmodes = 0;
            unsigned long long toks = 0;
            for (int w = 0; w < nwaves; ++w) {
                const uint32_t m = red[flip * 8 + w * 2], n = red[flip * 8 + w * 2 + 1];
                if (m > maxc) { maxc = m; nmodes = n; }
                else if (m == maxc) nmodes += n;
                toks += red_tok[flip * 4 + w];
            }
            flip ^= 1;
            do {                                                                     // every budget of this size (k > 0: maxc > 0)
                if (tid == 0) {
                    const int32_t b = ord[q];
                    if (tc) acc[b] += tc;
                    if (toks) acc[B + b] += toks;
                    if (tbin >= 0 && tc == maxc) {
                        if (nmodes < (uint32_t)TCL) tie[b * TCL + nmodes] += 1u;
                        else atomicAdd(&a.tie_hits[(int64_t)b * SCV_TIE_CLASSES + nmodes], 1ull);
                        if (a.per_resample) {
                            if (nmodes < (uint32_t)a.M) atomicAdd(&a.per_resample[((int64_t)rr * B + b) * a.M + nmodes], 1ull);
                            else atomicOr(a.err_flag, 2u);
                        }
                    }
                }
                ++q;
            } while (q < B && __builtin_amdgcn_readfirstlane(ks[q]) == k);
        }
        if (++since_flush == 0x7fffffffu) {                                          // (uniform) no 32-bit counter of the tie table wraps
            __syncthreads();
            flush_tie();
            since_flush = 0;
        }
        if (++rr == (int32_t)R) { rr = 0; ++p; fresh = true; }
        __syncthreads();                                                              // lane 0's tables, the words and the row before the next item
    }
    if (__ballot(bad) && lane == 0) atomicOr(a.err_flag, 1u);
    __syncthreads();
    flush_tie();
    if (tid < B) {
        if (a.truth_sum && acc[tid]) atomicAdd(&a.truth_sum[tid], acc[tid]);
        if (a.token_sum && acc[B + tid]) atomicAdd(&a.token_sum[tid], acc[B + tid]);
    }
}

}  // namespace scv
