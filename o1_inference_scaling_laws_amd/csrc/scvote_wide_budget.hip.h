// scvote_wide_budget.hip.h -- majority vote over the longest prefix of an ordering of a pool of up to 4096 samples that fits a TOKEN budget
// (scv_token_budget_wide_i32): a further body of scv_resample_prefix<false> (mode kResampleModeWideBudget), included by scvote_resample.hip.h
// behind scvote_wide.hip.h, whose sort, row encoder and item walk it reuses.
//
// The wide body sorts an ordering's N words in LDS and walks the sorted order budget by budget, k_b samples each.  Here budget b ends where the
// running token sum of the ordering would cross T_b.  Once the sort is done the 52 random bits of a word are dead, and a running sum of a row
// is below 4096 * 2^31 = 2^43: the sum takes their place, with the pool index still below it.  Per item:
//  * the words are built and sorted as in wide_body (SCV_ORDER_SHUFFLED: the same salt, stride and words, so the same orderings); in
//    SCV_ORDER_POOL word e is e and no sort runs.
//  * a lane takes a contiguous chunk of ceil(N / lanes) sorted words, gathers tokens[p, idx] from global memory (the row is at most 16 KiB that
//    the R items of a problem share: L1 / L2 hits) and parks each count in its word; the chunk sums are scanned over the wave (shuffles) and
//    across the waves through LDS -- the shape of the head-count scan of wide_encode_row_open, in int64 --, and a second pass over the chunk
//    rewrites every word as running sum << 12 | idx.  A negative count raises error bit 4 and is added as 0: the sums stay monotone and
//    inside their field, and no walk leaves the row.
//  * the budgets are sorted once per launch by (T_b, b) (int64 rank sort in LDS); lane q < B finds n_q = the number of words whose sum field
//    is <= T_q by binary search (64-bit signed compare: a negative budget finds none).  n_q is non-decreasing in q, so the segment walk of
//    wide_body applies unchanged: ONE histogram, a scan at each boundary.
//  * at a boundary the cell's tokens are the sum field of word n_q - 1 (no per-lane token accumulation), its votes n_q.  In pool order the
//    scan also carries the smallest modal bin, and lane 0 writes the 16-byte cell (as four words: scv_cell is 4-byte aligned) and its tokens;
//    the cells of empty prefixes are written before the walk.  Under SCV_FLAG_OPEN_DOMAIN the bin is the code (resample_min_mode).
//  * counter tables and their flush as in wide_body, with one more 64-bit table for the vote counts.
//
// LDS words: wide_budget_lds_words (scvote_dispatch.h).  N = 4096, B = 12: 32 KiB of words + 8 KiB of bins + 4 KiB of histogram + 6.8 KiB of
// tables (open domain: 8 KiB of histogram).
#pragma once

namespace scv {

// The prefix lengths of one item: every lane of the workgroup calls it behind the sort (shuffled != 0; the words' low 12 bits are pool indices) or
// with nothing in keys (pool order: word e is sample e).  Rewrites keys[e], e < N, as (running token sum << 12) | idx and writes nb[q] = the
// number of words whose sum is <= bud[q] for q < B; returns true when the lane met a negative token count (added as 0).  The caller's last
// reads of keys, wsum and nb lie behind a barrier; the results may be read on return.  A lane takes a contiguous chunk of the words, parks each
// token count in its word and sums the chunk; the sums are scanned over the wave (shuffles, int64) and across the waves through LDS (the shape
// of the head-count scan of wide_encode_row_open); a second pass over the chunk writes the running sums.  Outlined like that encoder, with its
// LDS pointers as 32-bit LDS addresses: the bodies of the kernel keep their register counts.
using lds_i64 = __attribute__((address_space(3))) long long;
__device__ __noinline__ bool wide_budget_scan(const int32_t* tok_row, int N_arg, int B_arg, int shuffled_arg, lds_u64* keys_l, lds_u64* wsum_l,
                                              lds_i64* bud_l, lds_i32* nb_l) {
    const int N = __builtin_amdgcn_readfirstlane(N_arg), B = __builtin_amdgcn_readfirstlane(B_arg);      // arguments of a real call arrive in VGPRs
    const bool shuffled = __builtin_amdgcn_readfirstlane(shuffled_arg) != 0;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    unsigned long long* keys = (unsigned long long*)keys_l;
    unsigned long long* wsum = (unsigned long long*)wsum_l;
    const long long* bud = (const long long*)bud_l;
    int32_t* nb = (int32_t*)nb_l;
    const int per = (N + lanes - 1) / lanes;
    const int e0 = tid * per < N ? tid * per : N, e1 = e0 + per < N ? e0 + per : N;
    bool neg = false;
    long long mine = 0;
    for (int e = e0; e < e1; ++e) {
        uint32_t idx = shuffled ? (uint32_t)keys[e] & (uint32_t)(SCV_WIDE_MAX_N - 1) : (uint32_t)e;
        idx = idx < (uint32_t)N ? idx : (uint32_t)N - 1u;                            // (the first N sorted words are the samples': idx is a pool index)
        int32_t t = tok_row[idx];
        if (t < 0) { neg = true; t = 0; }
        mine += t;
        keys[e] = ((unsigned long long)(uint32_t)t << 12) | idx;                    // parked for the second pass (only this lane reads or writes the chunk)
    }
    long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(incl, d, 64);
        if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[wave] = (unsigned long long)incl;
    __syncthreads();
    unsigned long long run = (unsigned long long)(incl - mine);
    for (int w = 0; w < nwaves; ++w) run += w < wave ? wsum[w] : 0ull;
    for (int e = e0; e < e1; ++e) {
        const unsigned long long w = keys[e];
        run += w >> 12;
        keys[e] = (run << 12) | (w & (unsigned long long)(SCV_WIDE_MAX_N - 1));
    }
    __syncthreads();
    if (tid < B) {                                                                  // n_q: the words whose sum is <= T_q (the sums do not decrease)
        const long long T = bud[tid];
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long)(keys[mid] >> 12) <= T) lo = mid + 1;
            else hi = mid;
        }
        nb[tid] = lo;
    }
    __syncthreads();
    return neg;
}

template <bool SHUF>
__device__ __forceinline__ void wide_budget_run(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int N = a.N, B = a.B;
    const int n2 = wide_pad(N), TCL = wide_tie_cols(N);
    constexpr bool shuffled = SHUF;
    const bool open = a.open_domain != 0;                                           // (uniform over the launch)
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);         // [n2] the sort words, then running sum << 12 | idx
    unsigned long long* acc = keys + n2;                                            // [B] truth-count sums | [B] token sums | [B] vote sums
    long long* bud = reinterpret_cast<long long*>(acc + 3 * B);                     // [32] budgets, ascending
    unsigned long long* wsum = reinterpret_cast<unsigned long long*>(bud + 32);     // [4] the waves' token sums
    uint32_t* hist = reinterpret_cast<uint32_t*>(wsum + 4);                         // [1024]; open domain: 16-bit counts, two per word
    uint32_t* tie = hist + wide_hist_words(N, open);                                // [B][TCL]
    uint32_t* red = tie + B * TCL;                                                  // [2][4][2] the waves' (largest scan key, bins at its count)
    int32_t* nb = reinterpret_cast<int32_t*>(red + 16);                             // [32] prefix lengths of the item, ascending
    int32_t* ord = nb + 32;                                                         // [32] the budgets' indices
    uint16_t* bins = reinterpret_cast<uint16_t*>(ord + 32);                         // [N] the row

    for (int i = tid; i < B * TCL; i += lanes) tie[i] = 0u;
    for (int i = tid; i < 3 * B; i += lanes) acc[i] = 0ull;                         // 3 B (up to 96) may exceed the lanes
    if (tid < B) {                                                                  // rank sort by (T_b, b)
        const long long t = a.budgets[tid];
        int rank = 0;
        for (int b = 0; b < B; ++b) {
            const long long tb = a.budgets[b];
            rank += (tb < t || (tb == t && b < tid)) ? 1 : 0;
        }
        bud[rank] = t;
        ord[rank] = tid;
    }
    __syncthreads();

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
    bool bad = false, neg = false, fresh = true;
    int32_t tbin = -1;
    int hw = kBins;                                                                 // live words of the histogram (open domain: ceil(D / 2), per problem)
    uint32_t since_flush = 0;
    for (int64_t it = it0; it < it1; ++it) {
        if (fresh) {                                                                // a new problem: its row, its truth (the last item's reads lie behind a barrier)
            const int32_t* row = a.pool + p * (int64_t)N;
            const int32_t t = a.truth[p];
            if (open) {                                                             // every bin, the truth's code and D anew: nothing of the last problem stays
                wide_encode_row_open(row, t, N, (lds_u64*)keys, (lds_u16*)bins, (lds_u32*)red);
                tbin = __builtin_amdgcn_readfirstlane((int32_t)red[8]);
                hw = (__builtin_amdgcn_readfirstlane((int32_t)red[9]) + 1) >> 1;     // (red is next written behind this item's barriers)
            } else {
                for (int e = tid; e < N; e += lanes) {
                    int32_t x = row[e];
                    if ((uint32_t)x >= (uint32_t)kBins) { bad = true; x = kBins - 1; }
                    bins[e] = (uint16_t)x;
                }
                tbin = (uint32_t)t < (uint32_t)kBins ? t : -1;
            }
            fresh = false;
        }
        if (shuffled) {
            const uint64_t s = mix64((a.seed ^ kWideSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
            const uint64_t base = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)SCV_WIDE_MAX_N + 1ull);
            for (int i = tid; i < n2; i += lanes)
                keys[i] = i < N ? ((mix64(base + kGolden * (uint64_t)i) & ~(uint64_t)(SCV_WIDE_MAX_N - 1)) | (uint64_t)i) : ~0ull;
        }
        for (int i = tid; i < hw; i += lanes) hist[i] = 0u;
        __syncthreads();
        if (shuffled) wide_sort(keys, n2, tid, lanes);
        neg |= wide_budget_scan(a.tokens + p * (int64_t)N, N, B, shuffled ? 1 : 0, (lds_u64*)keys, (lds_u64*)wsum, (lds_i64*)bud, (lds_i32*)nb);
        int q = 0;
        while (q < B && __builtin_amdgcn_readfirstlane(nb[q]) == 0) {                // empty prefixes: no hit, nothing to add; pool order: an empty cell
            if (!shuffled && tid == 0) {
                const int64_t cell = p * (int64_t)B + ord[q];
                if (a.cells_out) {
                    uint32_t* cw = reinterpret_cast<uint32_t*>(a.cells_out) + 4 * cell;
                    cw[0] = 0u; cw[1] = 0u; cw[2] = 0xffff0000u; cw[3] = 0u;           // (min_mode -1)
                }
                if (a.cell_tokens_out) a.cell_tokens_out[cell] = 0;
            }
            ++q;
        }
        int32_t at = 0;
        int flip = 0;
        while (q < B) {
            const int32_t k = __builtin_amdgcn_readfirstlane(nb[q]);
            for (int32_t e = at + tid; e < k; e += lanes) {
                uint32_t idx = (uint32_t)keys[e] & (uint32_t)(SCV_WIDE_MAX_N - 1);
                idx = idx < (uint32_t)N ? idx : (uint32_t)N - 1u;
                const uint32_t c = bins[idx];                                       // open domain: count c is half (c & 1) of word c >> 1
                __hip_atomic_fetch_add(&hist[open ? c >> 1 : c], open ? 1u << ((c & 1u) << 4) : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            at = k;
            __syncthreads();
            // a bin's scan key: count << 12 | 4095 - bin (a count is at most 4096, a bin at most 4095).  The largest key of the row is its largest
            // count at its SMALLEST bin, so one word carries both and the wave reduction is one maximum; a lane's bins ascend, so a key
            // above its best has a larger count, and two keys share a count exactly when they differ below bit 12.
            uint32_t best = 0, nm = 0;
            if (open) {                                                             // (a count of 0, the odd half of the last word too, never ties the largest: k > 0)
#pragma nounroll
                for (int i = tid; i < hw; i += lanes) {
                    const uint32_t w = hist[i];
                    const uint32_t k0 = ((w & 0xffffu) << 12) | (4095u - 2u * (uint32_t)i), k1 = ((w >> 16) << 12) | (4094u - 2u * (uint32_t)i);
                    if (k0 > best) { best = k0; nm = 1u; }
                    else if ((k0 ^ best) < 4096u) nm += 1u;
                    if (k1 > best) { best = k1; nm = 1u; }
                    else if ((k1 ^ best) < 4096u) nm += 1u;
                }
            } else {
#pragma nounroll
                for (int i = tid; i < kBins; i += lanes) {
                    const uint32_t kk = (hist[i] << 12) | (4095u - (uint32_t)i);
                    if (kk > best) { best = kk; nm = 1u; }
                    else if ((kk ^ best) < 4096u) nm += 1u;
                }
            }
            const uint32_t tc = tbin < 0 ? 0u : open ? (hist[tbin >> 1] >> ((tbin & 1) << 4)) & 0xffffu : hist[tbin];
            const uint32_t wbest = wave_max_u32(best);
            const uint32_t wnm = wave_sum_u32((best ^ wbest) < 4096u ? nm : 0u);
            if (lane == 0) {
                red[flip * 8 + wave * 2] = wbest;
                red[flip * 8 + wave * 2 + 1] = wnm;
            }
            __syncthreads();
            uint32_t top = 0, nmodes = 0;
            for (int w = 0; w < nwaves; ++w) {
                const uint32_t m = red[flip * 8 + w * 2], n = red[flip * 8 + w * 2 + 1];
                if ((m ^ top) < 4096u) { nmodes += n; top = m > top ? m : top; }
                else if (m > top) { top = m; nmodes = n; }
            }
            const uint32_t maxc = top >> 12, minb = 4095u - (top & 4095u);
            flip ^= 1;
            const unsigned long long toks = keys[k - 1] >> 12;                       // k > 0: the sum behind the prefix's last sample
            do {                                                                     // every budget of this length (k > 0: maxc > 0)
                if (tid == 0) {
                    const int32_t b = ord[q];
                    const bool hit = tbin >= 0 && tc == maxc;
                    if (tc) acc[b] += tc;
                    if (toks) acc[B + b] += toks;
                    acc[2 * B + b] += (unsigned long long)k;
                    if (hit && nmodes >= (uint32_t)SCV_TIE_CLASSES) {
                        atomicOr(a.err_flag, 2u);                                    // (open domain, D > 1024) no column for the class: counted nowhere
                    } else if (hit) {
                        if (nmodes < (uint32_t)TCL) tie[b * TCL + nmodes] += 1u;
                        else atomicAdd(&a.tie_hits[(int64_t)b * SCV_TIE_CLASSES + nmodes], 1ull);
                        if (a.per_resample) {
                            if (nmodes < (uint32_t)a.M) atomicAdd(&a.per_resample[((int64_t)rr * B + b) * a.M + nmodes], 1ull);
                            else atomicOr(a.err_flag, 2u);
                        }
                    }
                    if (!shuffled) {                                                 // the cell of the cache order, as the token-budget body writes it
                        const int64_t cell = p * (int64_t)B + b;
                        if (a.cells_out) {
                            uint32_t* cw = reinterpret_cast<uint32_t*>(a.cells_out) + 4 * cell;      // scv_cell: 4-byte aligned only
                            cw[0] = maxc;
                            cw[1] = tc;
                            cw[2] = nmodes | (minb << 16);                           // (minb < 4096: min_mode, the bin or the code)
                            cw[3] = hit ? 1u : 0u;
                        }
                        if (a.cell_tokens_out) a.cell_tokens_out[cell] = (int64_t)toks;
                    }
                }
                ++q;
            } while (q < B && __builtin_amdgcn_readfirstlane(nb[q]) == k);
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
    if (__ballot(neg) && lane == 0) atomicOr(a.err_flag, 16u);
    __syncthreads();
    flush_tie();
    if (tid < B) {
        if (a.truth_sum && acc[tid]) atomicAdd(&a.truth_sum[tid], acc[tid]);
        if (a.token_sum && acc[B + tid]) atomicAdd(&a.token_sum[tid], acc[B + tid]);
        if (a.vote_sum && acc[2 * B + tid]) atomicAdd(&a.vote_sum[tid], acc[2 * B + tid]);
    }
}

// (one instantiation per order, as in token_budget_body: with the order a run-time flag the body needs 76 VGPRs, split 69 and fewer)
__device__ __forceinline__ void wide_budget_body(const ResampleArgs& a, uint32_t* smem) {
    if (a.order == kOrderShuffled) wide_budget_run<true>(a, smem);
    else wide_budget_run<false>(a, smem);
}

}  // namespace scv
