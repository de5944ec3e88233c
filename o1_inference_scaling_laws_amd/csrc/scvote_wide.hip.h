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
//
// SCV_FLAG_OPEN_DOMAIN (a.open_domain, uniform over the launch): every int32 is a value of its own.  Once per problem of a workgroup's run the
// row is ENCODED by wide_encode_row_open: the words (value with its sign bit flipped << 32 | pool index) go through the same network, the heads
// of the runs of equal values are counted by a workgroup prefix sum, and every sample gets the rank of its value among the row's D distinct
// values as its 16-bit bin (D <= N <= 4096).  The histogram then has D live bins, not 1024: 16-bit counts, two per word (a count is at most N),
// ceil(D / 2) words zeroed per item and scanned per boundary -- a peaked pool of 50 values scans 25 words where the flag-off body scans 1024.
// D, the truth's code and the bins are rewritten for every problem; words of the histogram beyond ceil(D / 2) are neither zeroed nor read.
// A hit with n_modes >= SCV_TIE_CLASSES (only possible with D > 1024) has no column in tie_class_hits_out: error bit 1, counted nowhere.
//
// LDS words: wide_lds_words (scvote_dispatch.h).  N = 4096, B = 13: 32 KiB of words + 8 KiB of bins + 4 KiB of histogram + 6.6 KiB of tables
// (open domain: 8 KiB of histogram).
#pragma once

namespace scv {

constexpr uint64_t kWideSalt = 0x8EBC6AF09C88C6E3ull;

// The bitonic network over keys[0 .. n2), n2 a power of two: every compare-exchange of a stage is independent, lanes take them round-robin,
// one workgroup barrier per stage (the last one included: the sorted words may be read on return).  The caller's writes of keys lie behind a
// barrier of its own.
__device__ __forceinline__ void wide_sort(unsigned long long* keys, int n2, int tid, int lanes) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma nounroll
            for (int t = tid; t < (n2 >> 1); t += lanes) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));               // the pair (lo, lo + j)
                const unsigned long long x = keys[lo], y = keys[lo + j];
                if ((x > y) == ((lo & k) == 0)) { keys[lo] = y; keys[lo + j] = x; }
            }
            __syncthreads();
        }
    }
}

// SCV_FLAG_OPEN_DOMAIN: the whole workgroup encodes one row of N int32 into bins[i] = the rank of row[i] among the row's distinct values in
// ascending signed order.  meta[8] = the code of the truth t, or -1 when t is not in the row; meta[9] = D, the number of distinct values;
// meta[0 .. 4) is scratch (meta: the body's `red`, 16 words that no lane reads or writes between two items).  Every lane of the workgroup
// calls it; the caller's last reads of keys, bins and meta lie behind a barrier, and the results may be read on return.
// Sort (value ^ sign bit) << 32 | index, so equal values are runs; a lane takes a contiguous chunk of the sorted words, counts the heads of
// runs in it, the counts are scanned over the wave (DPP-free shuffles: once per problem) and across the waves through LDS, and a second pass
// over the chunk scatters head count - 1 to the samples' pool indices.  Outlined, with its LDS pointers as 32-bit LDS addresses: the bodies
// keep their register counts, and a flag-off launch never enters it.
using lds_u64 = __attribute__((address_space(3))) unsigned long long;
using lds_u16 = __attribute__((address_space(3))) uint16_t;
__device__ __noinline__ void wide_encode_row_open(const int32_t* row, int32_t t, int N_arg, lds_u64* keys_l, lds_u16* bins_l, lds_u32* meta_l) {
    const int N = __builtin_amdgcn_readfirstlane(N_arg);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int n2 = wide_pad(N);
    unsigned long long* keys = (unsigned long long*)keys_l;
    uint16_t* bins = (uint16_t*)bins_l;
    uint32_t* meta = (uint32_t*)meta_l;
    for (int i = tid; i < n2; i += lanes)                                           // (no sample's word is all-ones: its low half is an index)
        keys[i] = i < N ? (((unsigned long long)((uint32_t)row[i] ^ 0x80000000u) << 32) | (unsigned long long)i) : ~0ull;
    if (tid == 0) meta[8] = 0xffffffffu;
    __syncthreads();
    wide_sort(keys, n2, tid, lanes);
    const uint32_t* half = reinterpret_cast<const uint32_t*>(keys);                 // word e: half[2 e] the index, half[2 e + 1] the value
    const int per = (N + lanes - 1) / lanes;
    const int e0 = tid * per < N ? tid * per : N, e1 = e0 + per < N ? e0 + per : N;
    const uint32_t before = e0 > 0 && e0 < N ? half[2 * e0 - 1] : 0u;               // the value in front of the chunk (e = 0 is a head anyway)
    uint32_t heads = 0, prev = before;
    for (int e = e0; e < e1; ++e) {
        const uint32_t v = half[2 * e + 1];
        heads += (e == 0 || v != prev) ? 1u : 0u;
        prev = v;
    }
    uint32_t incl = heads;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += u;
    }
    if (lane == 63) meta[wave] = incl;
    __syncthreads();
    uint32_t code = incl - heads, D = 0;                                            // heads in front of the chunk ...
    for (int w = 0; w < nwaves; ++w) {
        const uint32_t c = meta[w];
        code += w < wave ? c : 0u;
        D += c;
    }
    code -= 1u;                                                                     // ... so its first word continues run `code` or opens `code + 1`
    const uint32_t tkey = (uint32_t)t ^ 0x80000000u;
    prev = before;
    for (int e = e0; e < e1; ++e) {
        const uint32_t v = half[2 * e + 1];
        uint32_t idx = half[2 * e] & (uint32_t)(SCV_WIDE_MAX_N - 1);
        idx = idx < (uint32_t)N ? idx : (uint32_t)N - 1u;                            // (the first N sorted words are the samples': idx is a pool index)
        if (e == 0 || v != prev) {
            code += 1u;
            if (v == tkey) meta[8] = code;                                          // one head at most holds the truth
        }
        prev = v;
        bins[idx] = (uint16_t)code;
    }
    if (tid == 0) meta[9] = D;
    __syncthreads();
}

__device__ __forceinline__ void wide_body(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int N = a.N, B = a.B;
    const int n2 = wide_pad(N), TCL = wide_tie_cols(N);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);         // [n2] the sort words
    unsigned long long* acc = keys + n2;                                            // [B] truth-count sums | [B] token sums
    unsigned long long* red_tok = acc + 2 * B;                                      // [2][4] the waves' token sums, slots alternate
    const bool open = a.open_domain != 0;                                           // (uniform over the launch)
    uint32_t* hist = reinterpret_cast<uint32_t*>(red_tok + 8);                      // [1024]; open domain: 16-bit counts, two per word
    uint32_t* tie = hist + wide_hist_words(N, open);                                // [B][TCL]
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
    int hw = kBins;                                                                 // live words of the histogram (open domain: ceil(D / 2), per problem)
    uint32_t since_flush = 0;
    for (int64_t it = it0; it < it1; ++it) {
        if (fresh) {                                                                // a new problem: its row, its truth (the last item's reads lie behind two barriers)
            const int32_t* row = a.pool + p * (int64_t)N;
            const int32_t t = a.truth[p];
            if (open) {                                                             // every bin, the truth's code and D anew: nothing of the last problem stays
                wide_encode_row_open(row, t, N, (lds_u64*)keys, (lds_u16*)bins, (lds_u32*)red);
                tbin = __builtin_amdgcn_readfirstlane((int32_t)red[8]);
                hw = (__builtin_amdgcn_readfirstlane((int32_t)red[9]) + 1) >> 1;     // (red is next written behind this item's first barrier)
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
        const uint64_t s = mix64((a.seed ^ kWideSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
        const uint64_t base = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)SCV_WIDE_MAX_N + 1ull);
        for (int i = tid; i < n2; i += lanes)
            keys[i] = i < N ? ((mix64(base + kGolden * (uint64_t)i) & ~(uint64_t)(SCV_WIDE_MAX_N - 1)) | (uint64_t)i) : ~0ull;
        for (int i = tid; i < hw; i += lanes) hist[i] = 0u;
        __syncthreads();
        wide_sort(keys, n2, tid, lanes);
        const int32_t* tok_row = a.tokens ? a.tokens + p * (int64_t)N : nullptr;
        long long tok = 0;
        int32_t at = 0;
        int q = q0, flip = 0;
        while (q < B) {
            const int32_t k = __builtin_amdgcn_readfirstlane(ks[q]);
            for (int32_t e = at + tid; e < k; e += lanes) {
                uint32_t idx = (uint32_t)keys[e] & (uint32_t)(SCV_WIDE_MAX_N - 1);
                idx = idx < (uint32_t)N ? idx : (uint32_t)N - 1u;                    // (the first N sorted words are the samples': idx is a pool index)
                const uint32_t c = bins[idx];                                       // open domain: count c is half (c & 1) of word c >> 1
                __hip_atomic_fetch_add(&hist[open ? c >> 1 : c], open ? 1u << ((c & 1u) << 4) : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (tok_row) tok += tok_row[idx];
            }
            at = k;
            __syncthreads();
            uint32_t mx = 0, nm = 0;
            if (open) {                                                             // (a count of 0, the odd half of the last word too, never ties the largest: k > 0)
#pragma nounroll
                for (int i = tid; i < hw; i += lanes) {
                    const uint32_t w = hist[i], c0 = w & 0xffffu, c1 = w >> 16;
                    if (c0 > mx) { mx = c0; nm = 1u; }
                    else if (c0 == mx) nm += 1u;
                    if (c1 > mx) { mx = c1; nm = 1u; }
                    else if (c1 == mx) nm += 1u;
                }
            } else {
#pragma nounroll
                for (int i = tid; i < kBins; i += lanes) {
                    const uint32_t c = hist[i];
                    if (c > mx) { mx = c; nm = 1u; }
                    else if (c == mx) nm += 1u;
                }
            }
            const uint32_t tc = tbin < 0 ? 0u : open ? (hist[tbin >> 1] >> ((tbin & 1) << 4)) & 0xffffu : hist[tbin];
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
                    if (tbin >= 0 && tc == maxc && nmodes >= (uint32_t)SCV_TIE_CLASSES) {
                        atomicOr(a.err_flag, 2u);                                    // (open domain, D > 1024) no column for the class: counted nowhere
                    } else if (tbin >= 0 && tc == maxc) {
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
