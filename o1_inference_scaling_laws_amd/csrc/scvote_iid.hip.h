// scvote_iid.hip.h -- majority vote over draws WITH replacement from one sample pool per problem (scv_iid_prefix_i32): a further body of
// scv_resample_prefix<false> (mode kResampleModeIid), included by scvote_resample.hip.h.
//
// The plug-in (bootstrap) estimate of maj@k: a problem's pool is taken for the model's answer distribution, k answers are drawn from it with
// replacement and voted on.  It is defined for any k -- the budgets are NOT clamped to N, only to SCV_IID_MAX_DRAWS = 65535 -- and its
// k -> infinity limit is the score of the vote over the whole pool.
//
// The walk is the shuffle's (scvote_resample.hip.h) without the shuffle: one lane per (problem, resample), rows staged per chunk by
// resample_encode_row (byte codes, the truth's code, the distinct count), budgets rank-sorted once per workgroup, uniform boundaries emitted
// by one ballot for n_modes == 1, LDS atomics for the rest, wave sums for the truth and token totals and one global atomic per hit into
// per_resample; the 32-bit tie table flushed every floor((2^32 - 1) / lanes) chunks.  What differs:
//  * a step is u = mix64(arg), arg += G; x = mulhi32(hi32(u), N); code = row[x]; c = ++cnt[code]; the running (maxc, nmodes); the truth
//    count; the optional token from the global row (read whatever the kernel's TOK, as the weighted body does).  No Fisher-Yates array.
//  * a count may reach 65535, so a lane owns 16-bit counts over the row's codes, laid out [slot / 2][lane] in words: half e of lane l lives
//    in word (e / 2) * lanes + l, and the 32 lanes of an access group hit 32 banks whatever code each drew.  A count never wraps: it is at
//    most the number of steps, and the walk ends at max_b k_b <= 65535.
//  * the stream of resample r starts at counter r * 65536 + 1, so the streams of different r never overlap (i + 1 <= 65535 < 65536).
//  * a budget above 65535 raises error bit 7 and the launch computes nothing (every workgroup sees the same list and leaves).
// n_modes <= min(distinct values, k) <= N, so the tie table stays [B][N + 1] in LDS.
#pragma once

namespace scv {

constexpr uint64_t kIidSalt = 0xA0761D6478BD642Full;
constexpr int32_t kIidMaxDraws = 65535;

__device__ __forceinline__ void iid_body(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int lanes_log2 = 31 - __clz(lanes);
    const int N = a.N, B = a.B, N4 = (N + 3) >> 2, TC = N + 1;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);         // [B] truth-count sums | [B] token sums
    uint32_t* tie = smem + 4 * B;                                                   // [B][N + 1]
    int32_t* ks = reinterpret_cast<int32_t*>(tie + B * TC);                         // [32] budgets, ascending
    int32_t* ord = ks + 32;                                                         // [32] their indices
    uint32_t* scr = reinterpret_cast<uint32_t*>(ord + 32);                          // [nwaves][64]
    int32_t* meta = reinterpret_cast<int32_t*>(scr + 64 * nwaves);                  // [np_max][2]
    uint32_t* rows = reinterpret_cast<uint32_t*>(meta + 2 * a.np_max);              // [np_max][N4]
    uint32_t* cnt = rows + a.np_max * N4;                                           // [(N + 1) / 2][lanes], two 16-bit counts per word
    uint16_t* cnt_h = reinterpret_cast<uint16_t*>(cnt);
    const uint8_t* rows_b = reinterpret_cast<const uint8_t*>(rows);

    for (int i = tid; i < B * TC; i += lanes) tie[i] = 0u;
    if (tid < 2 * B) acc[tid] = 0ull;
    if (tid < B) {                                                                  // rank sort: ties keep index order
        int32_t k = a.n_valid[tid];
        k = k < 0 ? 0 : k;
        int rank = 0;
        for (int b = 0; b < B; ++b) {
            int32_t kb = a.n_valid[b];
            kb = kb < 0 ? 0 : kb;
            rank += (kb < k || (kb == k && b < tid)) ? 1 : 0;
        }
        ks[rank] = k;
        ord[rank] = tid;
    }
    __syncthreads();
    const int32_t kmax = ks[B - 1];
    if (kmax > kIidMaxDraws) {                                                      // uniform over the launch: nothing is computed
        if (tid == 0) atomicOr(a.err_flag, 128u);
        return;
    }
    int q0 = 0;
    while (q0 < B && ks[q0] == 0) ++q0;                                              // empty cells: no hit, nothing to add
    const int64_t R = a.R, total = a.P * R;
    const int64_t nchunks = (total + lanes - 1) / lanes;
    const uint32_t lane_half = (uint32_t)tid << 1;
    bool bad = false, overflow = false;
    const int64_t epoch = (int64_t)(0xffffffffu / (uint32_t)lanes) * gridDim.x;    // as in scv_resample_prefix: no 32-bit counter wraps
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
        for (int w = 0; w < ((distinct + 1) >> 1); ++w) cnt[(w << lanes_log2) + tid] = 0u;
        const uint8_t* my_row = rows_b + (int64_t)row * N4 * 4;
        const int32_t* tok_row = a.tokens ? a.tokens + p * (int64_t)N : nullptr;
        const uint64_t s = mix64((a.seed ^ kIidSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
        uint64_t arg = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * 65536ull + 1ull);
        uint32_t maxc = 0, nmodes = 0, tc = 0;
        long long tok = 0;
        int q = q0;
        int32_t next_k = q < B ? ks[q] : 0x7fffffff;
        for (int32_t i = 0; i < kmax; ++i) {
            const uint64_t u = mix64(arg);
            arg += kGolden;
            const uint32_t x = mulhi32((uint32_t)(u >> 32), (uint32_t)N);
            const uint32_t code = (uint32_t)my_row[x];
            const uint32_t ac = ((code >> 1) << (lanes_log2 + 1)) + (code & 1u) + lane_half;
            const uint32_t c = (uint32_t)cnt_h[ac] + 1u;
            cnt_h[ac] = (uint16_t)c;
            if (c > maxc) { maxc = c; nmodes = 1u; }
            else if (c == maxc) nmodes += 1u;
            tc += (int32_t)code == tcode ? 1u : 0u;
            if (tok_row) tok += tok_row[x];
            if (i + 1 == next_k) {
                const bool hit = live && tcode >= 0 && tc == maxc;
                const uint32_t tcs = wave_sum_u32(live ? tc : 0u);
                const long long toks = tok_row ? wave_sum_i64(live ? tok : 0ll) : 0ll;
                const unsigned long long ones = __ballot(hit && nmodes == 1u);
                do {                                                                  // every budget of this size
                    const int32_t b = ord[q];
                    if (lane == 0) {
                        if (ones) atomicAdd(&tie[b * TC + 1], (uint32_t)__popcll(ones));
                        if (tcs) atomicAdd(&acc[b], (unsigned long long)tcs);
                        if (toks) atomicAdd(&acc[B + b], (unsigned long long)toks);
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
        if (a.token_sum && acc[B + tid]) atomicAdd(&a.token_sum[tid], acc[B + tid]);
    }
}

}  // namespace scv
