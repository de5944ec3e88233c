// scvote_weighted.hip.h -- weighted majority vote and best-of-N over the prefixes of a pool ordering (scv_weighted_prefix_i32): a third body
// of scv_resample_prefix<false> (mode kResampleModeWeighted; it reads the tokens itself when given, whatever the kernel's TOK), included by scvote_resample.hip.h.
//
// Every sample votes with an integer weight 0 .. SCV_WEIGHT_MAX (2^24 - 1).  W(v) of a prefix is the SUM (rule 0) or the MAXIMUM (rule 1) of
// the weights of its samples that voted v; the modes are the values with W(v) == max W > 0.  A lane keeps a uint32 total per row code in LDS,
// laid out [code][lane] (32 lanes of an access group hit 32 different banks whatever code each picked; N <= 256 weights below 2^24 sum below
// 2^32), and the mode statistics run in registers: with old = W(v) and new = old + w or max(old, w), nothing happens unless new > old; then
// new > top -> (top, n_modes) = (new, 1); new == top -> n_modes + 1.  A value that grows was strictly below `new` before, so it is never
// counted twice.  The truth's weight is a register (tw = W(truth code)); hit = tw == top > 0.
//
// Budgets are sample counts, the same for every lane, so the boundary is uniform and emitted as the shuffle body does (one ballot for the
// common n_modes == 1, LDS atomics for the rest, DPP sums of the tokens).  The rows are re-encoded per chunk (resample_encode_row); the same
// pass checks the weights' range (error bit 5).  Two layouts of a row, chosen by the host (a.wlds):
//   wlds    the row sits in LDS as words code | weight << 8, one LDS read per step gives both: R >= kWeightedLdsRowsMinR, where a chunk of
//           lanes touches at most lanes / R + 2 rows;
//   !wlds   byte codes in LDS, the weight is read from global memory (L1 / L2 hits, as the tokens are): few orderings per problem and the pool
//           order, where a chunk touches up to lanes + 1 rows and N words each would not fit beside the totals.
// SCV_ORDER_POOL: x = i, no Fisher-Yates array, one lane per problem, which also writes its cells (max_count = top W, truth_count = W(truth)).
// LDS per lane 4 N (totals) + N (Fisher-Yates, shuffled order) bytes: N = 128 -> 40 KiB per wave, N = 256 -> 80 KiB per wave.
#pragma once

namespace scv {

constexpr uint32_t kWeightMax = (1u << 24) - 1u;                                    // SCV_WEIGHT_MAX

template <bool SHUF, bool WLDS>
__device__ __forceinline__ void weighted_run(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int lanes_log2 = 31 - __clz(lanes);
    const int N = a.N, B = a.B, N4 = (N + 3) >> 2, TC = N + 1;
    const int RW = WLDS ? N : N4;                                                   // words of one staged row
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);          // [B] token sums
    uint32_t* tie = smem + 2 * B;                                                   // [B][N + 1]
    int32_t* ks = reinterpret_cast<int32_t*>(tie + B * TC);                         // [32] budgets, ascending
    int32_t* ord = ks + 32;                                                         // [32] their indices
    uint32_t* scr = reinterpret_cast<uint32_t*>(ord + 32);                          // [nwaves][64]
    int32_t* meta = reinterpret_cast<int32_t*>(scr + 64 * nwaves);                  // [np_max][2]
    uint32_t* rows = reinterpret_cast<uint32_t*>(meta + 2 * a.np_max);              // [np_max][RW]
    uint32_t* tot = rows + a.np_max * RW;                                           // [N][lanes]
    uint32_t* arr = tot + N * lanes;                                                // [N4][lanes] (shuffled order only)
    uint8_t* arr_b = reinterpret_cast<uint8_t*>(arr);
    const bool best_of = a.rule != 0;

    for (int i = tid; i < B * TC; i += lanes) tie[i] = 0u;
    if (tid < B) {                                                                  // rank sort: ties keep index order
        acc[tid] = 0ull;
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
    while (q0 < B && ks[q0] == 0) ++q0;                                              // empty prefixes: no hit, nothing to add
    const int64_t R = a.R, total = a.P * R;
    const int64_t nchunks = (total + lanes - 1) / lanes;
    const uint32_t lane_byte = (uint32_t)tid << 2;
    bool bad = false, wbad = false, overflow = false;
    const int64_t epoch = (int64_t)(0xffffffffu / (uint32_t)lanes) * gridDim.x;    // as in scv_resample_prefix: no 32-bit counter wraps
    for (int64_t c0 = blockIdx.x; c0 < nchunks; c0 += epoch) {
    const int64_t c1 = nchunks - c0 > epoch ? c0 + epoch : nchunks;
    for (int64_t chunk = c0; chunk < c1; chunk += gridDim.x) {
        const int64_t t0 = chunk * lanes;
        const int64_t p_lo = t0 / R;
        int64_t p_hi = (t0 + lanes - 1) / R;
        if (p_hi > a.P - 1) p_hi = a.P - 1;
        for (int64_t pl = wave; pl <= p_hi - p_lo; pl += nwaves) {
            uint32_t* rw = rows + pl * RW;
            bad |= resample_encode(a, p_lo + pl, reinterpret_cast<uint8_t*>(rw), meta + 2 * pl, scr + 64 * wave, lane);
            const int32_t* wrow = a.weights + (p_lo + pl) * (int64_t)N;
            // Word e takes the place of bytes 4 e .. 4 e + 3: the elements go from the top down, so that a word never lands on a byte code
            // that is still to be read (elements 64 k .. 64 k + 63 become bytes 256 k .. 256 k + 255, at or above every element below them),
            // and inside one group of 64 every byte is read before a word is written.
#pragma unroll
            for (int k = kResampleMaxN / 64 - 1; k >= 0; --k) {
                const int e = lane + 64 * k;
                uint32_t w = e < N ? (uint32_t)wrow[e] : 0u;
                if (w > kWeightMax) { wbad = true; w &= kWeightMax; }
                if (WLDS) {
                    const uint32_t word = e < N ? (uint32_t)reinterpret_cast<const uint8_t*>(rw)[e] | (w << 8) : 0u;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (e < N) rw[e] = word;
                }
            }
        }
        __syncthreads();
        const int64_t t = t0 + tid;
        const bool live = t < total;
        const int64_t p = (live ? t : total - 1) / R;
        const int32_t rr = SHUF ? (int32_t)((live ? t : total - 1) - p * R) : 0;
        const int32_t row = (int32_t)(p - p_lo);
        const int32_t tcode = meta[2 * row], distinct = meta[2 * row + 1];
        if (SHUF) for (int w = 0; w < N4; ++w) arr[(w << lanes_log2) + tid] = 0x03020100u + 0x04040404u * (uint32_t)w;
        for (int c = 0; c < distinct; ++c) tot[(c << lanes_log2) + tid] = 0u;
        const uint32_t* my_row = rows + (int64_t)row * RW;
        const uint8_t* my_row_b = reinterpret_cast<const uint8_t*>(my_row);
        const int32_t* w_base = a.weights + p_lo * (int64_t)N;                      // uniform bases, one 32-bit offset per lane
        const int32_t* tok_base = a.tokens ? a.tokens + p_lo * (int64_t)N : nullptr;
        const uint32_t row_off = (uint32_t)row * (uint32_t)N;
        uint64_t arg = 0;
        if (SHUF) {
            const uint64_t s = mix64((a.seed ^ kResampleSalt) + kGolden * (uint64_t)(a.p_offset + p + 1));
            arg = s + kGolden * ((uint64_t)(uint32_t)(a.r_begin + rr) * (uint64_t)N + 1ull);
        }
        uint32_t top = 0, nmodes = 0, tw = 0, min_x = 0, min_code = 0;            // min_x (pool order): a sample of the smallest modal value
        long long tok = 0;
        if (!SHUF && live) {                                                        // the cells of the empty prefixes
            for (int qq = 0; qq < q0; ++qq) {
                const int64_t cell = p * (int64_t)B + ord[qq];
                if (a.cells_out) {
                    uint32_t* cw = reinterpret_cast<uint32_t*>(a.cells_out) + 4 * cell;          // scv_cell: 4-byte aligned only
                    cw[0] = 0u; cw[1] = 0u; cw[2] = 0xffff0000u; cw[3] = 0u;
                }
                if (a.cell_tokens_out) a.cell_tokens_out[cell] = 0;
            }
        }
        int q = q0;
        int32_t next_k = q < B ? ks[q] : 0x7fffffff;
        for (int32_t i = 0; i < kmax; ++i) {
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
            uint32_t code, w;
            if (WLDS) { const uint32_t word = my_row[x]; code = word & 255u; w = word >> 8; }
            else { code = (uint32_t)my_row_b[x]; w = (uint32_t)w_base[row_off + x] & kWeightMax; }
            uint32_t* slot = tot + ((code << lanes_log2) + tid);
            const uint32_t old = *slot;
            const uint32_t now = best_of ? (w > old ? w : old) : old + w;
            if (now > old) {
                *slot = now;
                if (now > top) { top = now; nmodes = 1u; if (!SHUF) { min_x = x; min_code = code; } }
                else if (now == top) { nmodes += 1u; if (!SHUF && code < min_code) { min_x = x; min_code = code; } }
                if ((int32_t)code == tcode) tw = now;
            }
            if (tok_base) tok += tok_base[row_off + x];
            if (i + 1 == next_k) {
                const bool hit = live && tw != 0u && tw == top;
                const long long toks = tok_base ? wave_sum_i64(live ? tok : 0ll) : 0ll;
                const unsigned long long ones = __ballot(hit && nmodes == 1u);
                do {                                                                  // every budget of this size
                    const int32_t b = ord[q];
                    if (lane == 0) {
                        if (ones) atomicAdd(&tie[b * TC + 1], (uint32_t)__popcll(ones));
                        if (toks) atomicAdd(&acc[b], (unsigned long long)toks);
                    }
                    if (hit && nmodes != 1u) atomicAdd(&tie[b * TC + nmodes], 1u);
                    if (hit && a.per_resample) {
                        if (nmodes < (uint32_t)a.M) atomicAdd(&a.per_resample[((int64_t)rr * B + b) * a.M + nmodes], 1ull);
                        else overflow = true;
                    }
                    if (!SHUF && live) {
                        const int64_t cell = p * (int64_t)B + b;
                        if (a.cells_out) {
                            int32_t mm = -1;
                            if (top) mm = resample_min_mode(a, p, min_x, min_code);
                            uint32_t* cw = reinterpret_cast<uint32_t*>(a.cells_out) + 4 * cell;
                            cw[0] = top;
                            cw[1] = tw;
                            cw[2] = nmodes | ((uint32_t)(uint16_t)(int16_t)mm << 16);
                            cw[3] = hit ? 1u : 0u;
                        }
                        if (a.cell_tokens_out) a.cell_tokens_out[cell] = tok;
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
    if (__ballot(wbad) && lane == 0) atomicOr(a.err_flag, 32u);
    __syncthreads();
    for (int i = tid; i < B * TC; i += lanes) {
        const uint32_t v = tie[i];
        if (v) atomicAdd(&a.tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v);
    }
    if (tid < B && a.token_sum && acc[tid]) atomicAdd(&a.token_sum[tid], acc[tid]);
}

__device__ __forceinline__ void weighted_body(const ResampleArgs& a, uint32_t* smem) {
    if (a.order != kOrderShuffled) weighted_run<false, false>(a, smem);
    else if (a.wlds) weighted_run<true, true>(a, smem);
    else weighted_run<true, false>(a, smem);
}

}  // namespace scv
