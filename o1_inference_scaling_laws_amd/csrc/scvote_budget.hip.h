// scvote_budget.hip.h -- majority vote over the longest prefix of a pool ordering that fits a TOKEN budget (scv_token_budget_prefix_i32):
// the third body of scv_resample_prefix<true> (mode kResampleModeTokenBudget), included by scvote_resample.hip.h.
//
// The shuffle loop of scv_resample_prefix ends a vote after k_b samples, the same k_b for every lane, so its boundary test is uniform and a
// boundary is emitted with a wave ballot and DPP sums.  Here budget b ends where the lane's running token sum would cross T_b: step i reads
// the next sample's tokens t, and while spent + t > T_q the lane emits budget q from its current state (a prefix of i samples), then advances
// q.  Only then is the vote counted.  Boundaries are per lane, so emission is per lane: LDS atomics into the workgroup's tables (32-bit tie
// classes, 64-bit truth / token / vote sums) and, when requested, one global atomic per hit into per_resample.  A lane whose budgets are all
// emitted leaves the step loop; the wave leaves it when no lane is left or at i == N, and every budget still open then is emitted from the
// whole row.  Budgets are sorted once per workgroup (int64 rank sort); negative budgets are emitted empty at step 0, and so is every budget
// below the first sample's tokens.
//
// Everything else is the shuffle's: the rows are re-encoded per chunk (resample_encode_row), the lanes' Fisher-Yates and count byte arrays
// live in LDS as [slot / 4][lane] (counts only grow by one: the byte argument of scvote_resample.hip.h holds), the mode statistics run, and
// the 32-bit tie table is flushed into the int64 outputs every floor((2^32 - 1) / lanes) chunks (each lane emits each budget once per chunk).
// SCV_ORDER_POOL runs the same loop with x = i: no shuffle, no Fisher-Yates array in LDS; one lane per problem, which also writes its cells.
#pragma once

namespace scv {

// one wave checks the token row of problem p: true when a token count is negative (error bit 4: SCV_ERR_ARG)
__device__ __forceinline__ bool budget_row_has_negative(const int32_t* tok_row, int N, int lane) {
    bool neg = false;
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        if (e < N) neg = neg || tok_row[e] < 0;
    }
    return neg;
}

template <bool SHUF>
__device__ __forceinline__ void token_budget_run(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int lanes_log2 = 31 - __clz(lanes);
    const int N = a.N, B = a.B, N4 = (N + 3) >> 2, TC = N + 1;
    long long* bud = reinterpret_cast<long long*>(smem);                            // [32] budgets, ascending
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + 64);     // [B] truth-count sums | [B] token sums | [B] vote sums
    int32_t* ord = reinterpret_cast<int32_t*>(smem + 64 + 6 * B);                   // [32] the budgets' indices
    uint32_t* tie = reinterpret_cast<uint32_t*>(ord + 32);                          // [B][N + 1]
    uint32_t* scr = tie + B * TC;                                                   // [nwaves][64]
    int32_t* meta = reinterpret_cast<int32_t*>(scr + 64 * nwaves);                  // [np_max][2]
    uint32_t* rows = reinterpret_cast<uint32_t*>(meta + 2 * a.np_max);              // [np_max][N4]
    uint32_t* cnt = rows + a.np_max * N4;                                           // [N4][lanes]
    uint32_t* arr = cnt + N4 * lanes;                                               // [N4][lanes] (shuffled order only)
    uint8_t* arr_b = reinterpret_cast<uint8_t*>(arr);
    uint8_t* cnt_b = reinterpret_cast<uint8_t*>(cnt);
    const uint8_t* rows_b = reinterpret_cast<const uint8_t*>(rows);

    for (int i = tid; i < B * TC; i += lanes) tie[i] = 0u;
    for (int i = tid; i < 3 * B; i += lanes) acc[i] = 0ull;    // 3 B (up to 96) may exceed the lanes
    if (tid < B) {                                                                  // rank sort: ties keep index order
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
    const int64_t R = a.R, total = a.P * R;
    const int64_t nchunks = (total + lanes - 1) / lanes;
    const uint32_t lane_byte = (uint32_t)tid << 2;
    bool bad = false, neg = false, overflow = false;
    const int64_t epoch = (int64_t)(0xffffffffu / (uint32_t)lanes) * gridDim.x;    // as in scv_resample_prefix: no 32-bit counter wraps
    for (int64_t c0 = blockIdx.x; c0 < nchunks; c0 += epoch) {
    const int64_t c1 = nchunks - c0 > epoch ? c0 + epoch : nchunks;
    for (int64_t chunk = c0; chunk < c1; chunk += gridDim.x) {
        const int64_t t0 = chunk * lanes;
        const int64_t p_lo = t0 / R;
        int64_t p_hi = (t0 + lanes - 1) / R;
        if (p_hi > a.P - 1) p_hi = a.P - 1;
        for (int64_t pl = wave; pl <= p_hi - p_lo; pl += nwaves) {
            bad |= resample_encode(a, p_lo + pl, reinterpret_cast<uint8_t*>(rows + pl * N4), meta + 2 * pl, scr + 64 * wave, lane);
            neg |= budget_row_has_negative(a.tokens + (p_lo + pl) * (int64_t)N, N, lane);
        }
        __syncthreads();
        const int64_t t = t0 + tid;
        const bool live = t < total;
        const int64_t p = (live ? t : total - 1) / R;
        const int32_t rr = SHUF ? (int32_t)((live ? t : total - 1) - p * R) : 0;
        const int32_t row = (int32_t)(p - p_lo);
        const int32_t tcode = meta[2 * row], distinct = meta[2 * row + 1];
        if (SHUF) for (int w = 0; w < N4; ++w) arr[(w << lanes_log2) + tid] = 0x03020100u + 0x04040404u * (uint32_t)w;
        for (int w = 0; w < ((distinct + 3) >> 2); ++w) cnt[(w << lanes_log2) + tid] = 0u;
        const uint8_t* my_row = rows_b + (int64_t)row * N4 * 4;
        const int32_t* tok_row = a.tokens + p * (int64_t)N;
        uint64_t arg = 0;
        if (SHUF) {
            const uint64_t s = mix64((a.seed ^ kResampleSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
            arg = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)N + 1ull);
        }
        uint32_t maxc = 0, nmodes = 0, tc = 0, min_x = 0;                         // min_x (pool order): a sample of the smallest modal value
        long long spent = 0;
        int q = live ? 0 : B;                                                       // a lane past the end emits nothing
        long long next_t = q < B ? bud[q] : 0;
        // budget ord[q] from the lane's state: a prefix of n samples, `spent` tokens
        auto emit = [&](int32_t n) {
            const int32_t b = ord[q];
            const bool hit = tc != 0u && tc == maxc;
            if (hit) {
                atomicAdd(&tie[b * TC + nmodes], 1u);
                if (a.per_resample) {
                    if (nmodes < (uint32_t)a.M) atomicAdd(&a.per_resample[((int64_t)rr * B + b) * a.M + nmodes], 1ull);
                    else overflow = true;
                }
            }
            if (tc) atomicAdd(&acc[b], (unsigned long long)tc);
            if (spent) atomicAdd(&acc[B + b], (unsigned long long)spent);
            if (n) atomicAdd(&acc[2 * B + b], (unsigned long long)n);
            if (!SHUF) {
                const int64_t cell = p * (int64_t)B + b;
                if (a.cells_out) {
                    int32_t mm = -1;
                    if (maxc) mm = resample_min_mode(a, p, min_x, (uint32_t)my_row[min_x]);
                    uint32_t* cw = reinterpret_cast<uint32_t*>(a.cells_out) + 4 * cell;      // scv_cell: 4-byte aligned only
                    cw[0] = maxc;
                    cw[1] = tc;
                    cw[2] = nmodes | ((uint32_t)(uint16_t)(int16_t)mm << 16);
                    cw[3] = hit ? 1u : 0u;
                }
                if (a.cell_tokens_out) a.cell_tokens_out[cell] = spent;
            }
            ++q;
            next_t = q < B ? bud[q] : 0;
        };
        int32_t i = 0;
        for (; i < N && q < B; ++i) {
            uint32_t x = (uint32_t)i;
            if (SHUF) {
                const uint64_t u = mix64(arg);
                arg += kGolden;
                const uint32_t j = (uint32_t)i + mulhi32((uint32_t)(u >> 32), (uint32_t)(N - i));
                const uint32_t ai = arr_b[resample_byte((uint32_t)i, lanes_log2, lane_byte)];
                const uint32_t aj = resample_byte(j, lanes_log2, lane_byte);
                x = arr_b[aj];
                arr_b[aj] = (uint8_t)ai;
            }
            const long long after = spent + (long long)tok_row[x];
            while (q < B && after > next_t) emit(i);
            if (q == B) break;                                                      // every budget emitted: the lane idles
            const uint32_t code = (uint32_t)my_row[x];
            const uint32_t ac = resample_byte(code, lanes_log2, lane_byte);
            const uint32_t c = (uint32_t)cnt_b[ac] + 1u;
            cnt_b[ac] = (uint8_t)c;
            if (c > maxc) { maxc = c; nmodes = 1u; if (!SHUF) min_x = x; }
            else if (c == maxc) { nmodes += 1u; if (!SHUF && code < (uint32_t)my_row[min_x]) min_x = x; }
            tc += (int32_t)code == tcode ? 1u : 0u;
            spent = after;
        }
        while (q < B) emit(i);                                                      // the whole row fits what is left
        __syncthreads();                                                            // the rows are rewritten by the next chunk
    }
    if (c1 < nchunks) {                                                             // another epoch follows (uniform)
        for (int i = tid; i < B * TC; i += lanes) {
            const uint32_t v = tie[i];
            if (v) { atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v); tie[i] = 0u; }
        }
        __syncthreads();
    }
    }
    if (__ballot(bad) && lane == 0) atomicOr(a.err_flag, 1u);
    if (__ballot(overflow) && lane == 0) atomicOr(a.err_flag, 2u);
    if (__ballot(neg) && lane == 0) atomicOr(a.err_flag, 16u);
    __syncthreads();
    for (int i = tid; i < B * TC; i += lanes) {
        const uint32_t v = tie[i];
        if (v) atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v);
    }
    if (tid < B) {
        if (a.truth_sum && acc[tid]) atomicAdd(&a.truth_sum[tid], acc[tid]);
        if (a.token_sum && acc[B + tid]) atomicAdd(&a.token_sum[tid], acc[B + tid]);
        if (a.vote_sum && acc[2 * B + tid]) atomicAdd(&a.vote_sum[tid], acc[2 * B + tid]);
    }
}

__device__ __forceinline__ void token_budget_body(const ResampleArgs& a, uint32_t* smem) {
    if (a.order == kOrderShuffled) token_budget_run<true>(a, smem);
    else token_budget_run<false>(a, smem);
}

}  // namespace scv
