// scvote_adaptive.hip.h -- majority vote that samples until a stopping rule says the vote is settled (scv_adaptive_prefix_i32): a further
// body of scv_resample_prefix<true> (mode kResampleModeAdaptive), included by scvote_resample.hip.h.
//
// The walk is the token-budget body's (scvote_budget.hip.h): one lane per (problem, ordering), per step one shuffle step, the code byte of
// the drawn sample, its count byte in LDS, the running mode statistics (maxc, nmodes, tc).  What ends a vote here is not a budget but the
// state of the vote itself, so the lane also keeps the runner-up count `sec`, valid whenever the mode is unique:
//   c > maxc:  the value that rises was a mode.  If it was one of several, the others stay behind at the old maxc: sec = old maxc.  If it was
//              the only one, nothing below it moved: sec stays.
//   c < maxc:  a value below the top rose to c: sec = max(sec, c).
//   c == maxc: one more mode; sec is not read while nmodes >= 2, and the next c > maxc sets it.
// With c1 = maxc and c2 = nmodes >= 2 ? maxc : sec, rule b stops after the n-th sample when c1 >= need[b][c2], or (SCV_STOP_DECIDED) when
// c1 - c2 > n_max_b - n, or at n == n_max_b.  Every lane holds a 32-bit mask of its open rules and tests each of them after every sample
// (need as uint16 [B][N + 1] in LDS, the caps beside it); a rule that stops is emitted from the lane's state -- LDS atomics into the 32-bit
// tie-class and stop-length tables, 64-bit truth and token sums (the vote sum is read off the stop table when it is flushed), one global atomic per hit into per_resample when requested -- and
// leaves the mask.  The test runs before each step, on the state after n = 0, 1, ... samples, so a rule of cap 0 is emitted empty by the same
// code (need is clamped to 1 .. N + 1 in LDS: nothing else stops at n = 0, and 0 and 1 stop alike from n = 1 on).  The lane leaves the
// step loop when its mask is empty, the wave when no lane is left.  Both 32-bit tables are flushed into the int64 outputs every
// floor((2^32 - 1) / lanes) chunks (a lane adds at most one to a counter per chunk).  SCV_ORDER_POOL runs the same loop with x = i: one
// lane per problem, which also writes its cells.
#pragma once

namespace scv {

template <bool SHUF>
__device__ __forceinline__ void adaptive_run(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int lanes_log2 = 31 - __clz(lanes);
    const int N = a.N, B = a.B, N4 = (N + 3) >> 2, TC = N + 1;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);          // [B] truth-count sums | [B] token sums | [B] vote sums
    int32_t* capn = reinterpret_cast<int32_t*>(smem + 6 * B);                       // [32] n_max_b
    uint32_t* rmask = reinterpret_cast<uint32_t*>(capn + 32);                       // [0]: the rules with SCV_STOP_DECIDED
    uint32_t* tie = rmask + 2;                                                      // [B][N + 1]
    uint32_t* stop = tie + B * TC;                                                  // [B][N + 1]
    uint16_t* need = reinterpret_cast<uint16_t*>(stop + B * TC);                    // [B][N + 1]
    uint32_t* scr = stop + B * TC + ((B * TC + 1) >> 1);                            // [nwaves][64]
    int32_t* meta = reinterpret_cast<int32_t*>(scr + 64 * nwaves);                  // [np_max][2]
    uint32_t* rows = reinterpret_cast<uint32_t*>(meta + 2 * a.np_max);              // [np_max][N4]
    uint32_t* cnt = rows + a.np_max * N4;                                           // [N4][lanes]
    uint32_t* arr = cnt + N4 * lanes;                                               // [N4][lanes] (shuffled order only)
    uint8_t* arr_b = reinterpret_cast<uint8_t*>(arr);
    uint8_t* cnt_b = reinterpret_cast<uint8_t*>(cnt);
    const uint8_t* rows_b = reinterpret_cast<const uint8_t*>(rows);

    for (int i = tid; i < B * TC; i += lanes) {
        tie[i] = 0u;
        stop[i] = 0u;
        const int32_t v = a.need[i];
        need[i] = (uint16_t)(v < 1 ? 1 : (v > TC ? TC : v));      // c1 >= 1 once a sample is counted: 0 and 1 stop alike
    }
    for (int i = tid; i < 3 * B; i += lanes) acc[i] = 0ull;    // 3 B (up to 96) may exceed the lanes
    if (tid < 64) {                                            // the first wave: caps and flags, one rule per lane
        int32_t k = 0;
        uint32_t f = 0;
        if (tid < B) {
            k = a.cap[tid];
            k = k < 0 ? 0 : (k > N ? N : k);
            f = a.rule_flags ? (uint32_t)a.rule_flags[tid] : 0u;
            if (f & ~1u) atomicOr(a.err_flag, 64u);             // an unknown flag bit: SCV_ERR_ARG
        }
        if (tid < 32) capn[tid] = k;
        const unsigned long long decided = __ballot((f & 1u) != 0u);
        if (tid == 0) rmask[0] = (uint32_t)decided;
    }
    __syncthreads();
    const uint32_t m_dec = rmask[0];
    const uint32_t m_all = B == 32 ? 0xffffffffu : (1u << B) - 1u;
    const int64_t R = a.R, total = a.P * R;
    const int64_t nchunks = (total + lanes - 1) / lanes;
    const uint32_t lane_byte = (uint32_t)tid << 2;
    const int64_t epoch = (int64_t)(0xffffffffu / (uint32_t)lanes) * gridDim.x;    // as in scv_resample_prefix: no 32-bit counter wraps
    for (int64_t c0 = blockIdx.x; c0 < nchunks; c0 += epoch) {
    const int64_t c1 = nchunks - c0 > epoch ? c0 + epoch : nchunks;
    for (int64_t chunk = c0; chunk < c1; chunk += gridDim.x) {
        const int64_t t0 = chunk * lanes;
        const int64_t p_lo = t0 / R;
        int64_t p_hi = (t0 + lanes - 1) / R;
        if (p_hi > a.P - 1) p_hi = a.P - 1;
        for (int64_t pl = wave; pl <= p_hi - p_lo; pl += nwaves) {                  // the error bits are raised where they are found: no lane carries them
            const bool bad = resample_encode(a, p_lo + pl, reinterpret_cast<uint8_t*>(rows + pl * N4), meta + 2 * pl, scr + 64 * wave, lane);
            if (__ballot(bad) && lane == 0) atomicOr(a.err_flag, 1u);
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
        const int32_t* tok_row = a.tokens ? a.tokens + p * (int64_t)N : nullptr;
        uint64_t arg = 0;
        if (SHUF) {
            const uint64_t s = mix64((a.seed ^ kResampleSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
            arg = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)N + 1ull);
        }
        uint32_t maxc = 0, nmodes = 0, tc = 0, sec = 0, min_x = 0;                // min_x (pool order): a sample of the smallest modal value
        long long spent = 0;
        // rule b from the lane's state: n samples counted, `spent` tokens
        auto emit = [&](int32_t b, int32_t n) {
            const bool hit = tc != 0u && tc == maxc;
            if (hit) {
                atomicAdd(&tie[b * TC + nmodes], 1u);
                if (a.per_resample) {
                    if (nmodes < (uint32_t)a.M) atomicAdd(&a.per_resample[((int64_t)rr * B + b) * a.M + nmodes], 1ull);
                    else atomicOr(a.err_flag, 2u);
                }
            }
            atomicAdd(&stop[b * TC + n], 1u);
            atomicAdd(&acc[b], (unsigned long long)tc);
            atomicAdd(&acc[B + b], (unsigned long long)spent);
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
                if (a.cell_votes_out) a.cell_votes_out[cell] = n;
            }
        };
        uint32_t open = live ? m_all : 0u;                                          // a lane past the end emits nothing
        for (int32_t n = 0;; ++n) {
            // the open rules against the state after n samples (n = 0: only a cap of 0 stops, need is >= 1 in LDS)
            const uint32_t c2 = nmodes >= 2u ? maxc : sec;
            for (uint32_t m = open; m; m &= m - 1u) {
                const int32_t b = __ffs((int)m) - 1;
                const int32_t left = capn[b] - n;
                const bool decided = ((m_dec >> b) & 1u) && (int32_t)(maxc - c2) > left;
                if (maxc >= (uint32_t)need[b * TC + c2] || decided || left == 0) {
                    emit(b, n);
                    open &= ~(1u << b);
                }
            }
            if (!open) break;                                                       // every cap is <= N: nothing is open at n == N
            uint32_t x = (uint32_t)n;
            if (SHUF) {
                const uint64_t u = mix64(arg);
                arg += kGolden;
                const uint32_t j = (uint32_t)n + mulhi32((uint32_t)(u >> 32), (uint32_t)(N - n));
                const uint32_t ai = arr_b[resample_byte((uint32_t)n, lanes_log2, lane_byte)];
                const uint32_t aj = resample_byte(j, lanes_log2, lane_byte);
                x = arr_b[aj];
                arr_b[aj] = (uint8_t)ai;
            }
            const uint32_t code = (uint32_t)my_row[x];
            const uint32_t ac = resample_byte(code, lanes_log2, lane_byte);
            const uint32_t c = (uint32_t)cnt_b[ac] + 1u;
            cnt_b[ac] = (uint8_t)c;
            if (c > maxc) { if (nmodes > 1u) sec = maxc; maxc = c; nmodes = 1u; if (!SHUF) min_x = x; }
            else if (c == maxc) { nmodes += 1u; if (!SHUF && code < (uint32_t)my_row[min_x]) min_x = x; }
            else sec = c > sec ? c : sec;
            tc += (int32_t)code == tcode ? 1u : 0u;
            if (tok_row) spent += (long long)tok_row[x];
        }
        __syncthreads();                                                            // the rows are rewritten by the next chunk
    }
    if (c1 < nchunks) {                                                             // another epoch follows (uniform)
        for (int i = tid; i < B * TC; i += lanes) {
            const uint32_t v = tie[i], s = stop[i];
            if (v) { atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v); tie[i] = 0u; }
            if (s) {                                                               // the votes drawn are those the stop table counts
                atomicAdd(&acc[2 * B + i / TC], (unsigned long long)s * (unsigned)(i % TC));
                if (a.stop_hist) atomicAdd(&a.stop_hist[i], (unsigned long long)s);
                stop[i] = 0u;
            }
        }
        __syncthreads();
    }
    }
    __syncthreads();
    for (int i = tid; i < B * TC; i += lanes) {
        const uint32_t v = tie[i], s = stop[i];
        if (v) atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v);
        if (s) {
            atomicAdd(&acc[2 * B + i / TC], (unsigned long long)s * (unsigned)(i % TC));
            if (a.stop_hist) atomicAdd(&a.stop_hist[i], (unsigned long long)s);
        }
    }
    __syncthreads();
    if (tid < B) {
        if (a.truth_sum && acc[tid]) atomicAdd(&a.truth_sum[tid], acc[tid]);
        if (a.token_sum && acc[B + tid]) atomicAdd(&a.token_sum[tid], acc[B + tid]);
        if (a.vote_sum && acc[2 * B + tid]) atomicAdd(&a.vote_sum[tid], acc[2 * B + tid]);
    }
}

__device__ __forceinline__ void adaptive_body(const ResampleArgs& a, uint32_t* smem) {
    if (a.order == kOrderShuffled) adaptive_run<true>(a, smem);
    else adaptive_run<false>(a, smem);
}

}  // namespace scv
