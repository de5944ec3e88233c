// scvote_shortest.hip.h -- short-m@k: majority vote over the m SHORTEST of the first k samples of a pool ordering (scv_shortest_prefix_i32):
// a further body of scv_resample_prefix<true> (mode kResampleModeShortest), included by scvote_resample.hip.h.
//
// k samples are launched in parallel, the m that finish first (fewest tokens; ties by pool index) vote, the others are cut off when the m-th
// finishes.  The kept set V is a function of the SET of the first k samples, so the walk keeps no vote state at all:
//  * per chunk, the wave that encodes a row (resample_encode) also ranks its tokens: trank[e] = the number of samples j with
//    (tokens[j], j) < (tokens[e], e), a permutation of 0 .. N - 1, counted in registers with the readlane broadcast loop of open_count_below.
//    A row in LDS is three byte arrays: the codes, trank, and the inverse by_rank.
//  * per lane, [word][lane] in LDS as in the siblings: the Fisher-Yates array of pool indices (shuffled order only), a presence bitmap over
//    token ranks (ceil(N / 32) words) and the count bytes over codes.  A shuffle step draws x and sets bit trank[x]; no vote is counted.
//  * budgets are sorted once per workgroup by (k, m, index).  At a boundary i + 1 = k the lane zeroes its counts and walks the set bits of its
//    bitmap in ascending rank: idx = by_rank[r], the code from the row, the count byte and the running (max, n_modes, truth count), the token
//    from global memory.  Budgets of one k are emitted in ascending m out of ONE walk: the trip count between two of them, m_b - m_(b-1), is
//    the same for every lane.  The last idx walked gives t_(m), the latency; spent = voted + (k - m) * t_(m) in int64.
//  * emission is the shuffle's (scvote_resample.hip.h): a ballot for n_modes == 1, an LDS atomic for the rest, DPP sums of the truth counts
//    and the three token sums into the workgroup's 64-bit tables, one global atomic per hit into per_resample when requested; the 32-bit tie
//    table is flushed every floor((2^32 - 1) / lanes) chunks.
// Count bytes: counts only grow by one inside a walk, and 256 arises only as the last of 256 steps of one k -- never read back from its byte
// (the argument of scvote_resample.hip.h); the next boundary zeroes the bytes first.  SCV_ORDER_POOL runs the same loop with x = i: one lane
// per problem, which also writes its cells.  No array in registers is indexed dynamically.
#pragma once

namespace scv {

// one broadcast step of the token ranking: token j = 64 KK + jl goes to a scalar register, every lane counts it against its NK tokens (element
// e = 64 k + lane).  (tj, j) < (te, e): for k > KK j < e always, for k < KK never, and for k == KK one 64-bit compare of tj * 64 + jl against
// mine = te * 64 + lane.
template <int NK, int KK>
__device__ __forceinline__ void shortest_rank_step(int32_t src, int jl, long long mine, const int32_t (&key)[kResampleMaxN / 64], int32_t (&lt)[kResampleMaxN / 64]) {
    const int32_t s = __builtin_amdgcn_readlane(src, jl);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (k > KK) lt[k] += s <= key[k] ? 1 : 0;
        else if (k < KK) lt[k] += s < key[k] ? 1 : 0;
        else lt[k] += ((long long)s * 64 + jl) < mine ? 1 : 0;
    }
}
template <int NK, int KK>
__device__ __forceinline__ void shortest_rank_reg(const int32_t (&key)[kResampleMaxN / 64], int32_t (&lt)[kResampleMaxN / 64], int n) {
    const long long mine = (long long)key[KK] * 64 + ((int)threadIdx.x & 63);
#pragma nounroll
    for (int jl = 0; jl < n; ++jl) shortest_rank_step<NK, KK>(key[KK], jl, mine, key, lt);
}
// lt[k] = samples in front of element 64 k + lane in (tokens, index) order, for a row of N tokens in NK registers, 64 (NK - 1) < N <= 64 NK
template <int NK>
__device__ __forceinline__ void shortest_rank_below(const int32_t (&key)[kResampleMaxN / 64], int32_t (&lt)[kResampleMaxN / 64], int N) {
    const int tail = N - 64 * (NK - 1);
    if constexpr (NK > 1) shortest_rank_reg<NK, 0>(key, lt, 64);
    if constexpr (NK > 2) shortest_rank_reg<NK, 1>(key, lt, 64);
    if constexpr (NK > 3) shortest_rank_reg<NK, 2>(key, lt, 64);
    shortest_rank_reg<NK, NK - 1>(key, lt, tail);
}

// One wave ranks the token row of a problem: trank[e] (bytes) and its inverse by_rank[trank[e]] = e.  Returns true when a token count is
// negative (error bit 4).  Outlined like resample_encode_row_open, LDS pointers as 32-bit LDS addresses: the bodies keep their registers.
__device__ __noinline__ bool shortest_rank_row(const int32_t* tok_row, int N_arg, lds_u8* trank_l, lds_u8* by_rank_l) {
    const int N = __builtin_amdgcn_readfirstlane(N_arg);
    const int lane = (int)threadIdx.x & 63;
    int32_t key[kResampleMaxN / 64], lt[kResampleMaxN / 64];
    bool neg = false;
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        key[k] = e < N ? tok_row[e] : 0;
        neg = neg || key[k] < 0;
        lt[k] = 0;
    }
    const int nk = (N + 63) >> 6;
    if (nk == 1) shortest_rank_below<1>(key, lt, N);
    else if (nk == 2) shortest_rank_below<2>(key, lt, N);
    else if (nk == 3) shortest_rank_below<3>(key, lt, N);
    else shortest_rank_below<4>(key, lt, N);
#pragma unroll
    for (int k = 0; k < kResampleMaxN / 64; ++k) {
        const int e = lane + 64 * k;
        if (e < N) {                                                                // lt[k] < N: N - 1 other samples were counted
            trank_l[e] = (uint8_t)lt[k];
            by_rank_l[lt[k]] = (uint8_t)e;
        }
    }
    return neg;
}

// The kernel's argument block, read again from the kernarg segment.  The outputs are touched at a hit, at a cell and in the flushes; loaded
// where they are used they are scalar loads that hit the constant cache, kept from the top of the kernel they are two dozen scalar
// registers that the allocator parks in VGPR lanes for the whole walk -- a third VGPR of such lanes, and the seventh wave per SIMD.
using kernarg_args = const ResampleArgs __attribute__((address_space(4)));
__device__ __forceinline__ kernarg_args* shortest_args_again() {
    kernarg_args* ka = (kernarg_args*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));                                                     // not the loads of the kernel's top again
    return ka;
}

template <bool SHUF>
__device__ __forceinline__ void shortest_run(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lanes = (int)blockDim.x, nwaves = lanes >> 6;
    const int lanes_log2 = 31 - __clz(lanes);
    const int N = a.N, B = a.B, N4 = (N + 3) >> 2, NW = (N + 31) >> 5, TC = N + 1;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);          // [B] truth counts | [B] voted | [B] spent | [B] latency
    uint32_t* tie = smem + 8 * B;                                                   // [B][N + 1]
    int32_t* ks = reinterpret_cast<int32_t*>(tie + B * TC);                         // [32] k_b, ascending
    int32_t* ms = ks + 32;                                                          // [32] m_b, ascending inside one k
    int32_t* ord = ms + 32;                                                         // [32] the budgets' indices
    uint32_t* scr = reinterpret_cast<uint32_t*>(ord + 32);                          // [nwaves][64]
    int32_t* meta = reinterpret_cast<int32_t*>(scr + 64 * nwaves);                  // [np_max][2]
    uint32_t* rows = reinterpret_cast<uint32_t*>(meta + 2 * a.np_max);              // [np_max][3][N4]: codes | trank | by_rank
    uint32_t* cnt = rows + a.np_max * 3 * N4;                                       // [N4][lanes]
    uint32_t* bits = cnt + N4 * lanes;                                              // [NW][lanes]
    uint32_t* arr = bits + NW * lanes;                                              // [N4][lanes] (shuffled order only)
    uint8_t* arr_b = reinterpret_cast<uint8_t*>(arr);
    uint8_t* cnt_b = reinterpret_cast<uint8_t*>(cnt);
    const uint8_t* rows_b = reinterpret_cast<const uint8_t*>(rows);

    for (int i = tid; i < B * TC; i += lanes) tie[i] = 0u;
    for (int i = tid; i < 4 * B; i += lanes) acc[i] = 0ull;    // 4 B (up to 128) may exceed the lanes
    if (tid < B) {                                                                  // rank sort by (k, m): ties keep index order
        auto km = [&](int b) {
            int32_t k = a.n_valid[b], m = a.m_keep[b];
            k = k < 0 ? 0 : (k > N ? N : k);
            m = m < 0 ? 0 : (m > k ? k : m);
            return (k << 9) | m;                                                    // k, m <= 256
        };
        const int32_t mine = km(tid);
        int rank = 0;
        for (int b = 0; b < B; ++b) {
            const int32_t o = km(b);
            rank += (o < mine || (o == mine && b < tid)) ? 1 : 0;
        }
        ks[rank] = mine >> 9;
        ms[rank] = mine & 511;
        ord[rank] = tid;
    }
    __syncthreads();
    // what every lane reads from the sorted budgets is the same: it goes to scalar registers, and the loops it bounds are scalar loops
    const int32_t kmax = __builtin_amdgcn_readfirstlane(ks[B - 1]);
    int q0 = 0;
    while (q0 < B && __builtin_amdgcn_readfirstlane(ks[q0]) == 0) ++q0;                                              // empty cells: nothing to add (pool order: cells to write)
    const int64_t R = a.R, total = a.P * R;
    const int64_t nchunks = (total + lanes - 1) >> lanes_log2;                     // (the workgroup is a power of two)
    const uint32_t lane_byte = (uint32_t)tid << 2;
    const int64_t epoch = (int64_t)(0xffffffffu / (uint32_t)lanes) * gridDim.x;    // as in scv_resample_prefix: no 32-bit counter wraps
    for (int64_t c0 = blockIdx.x; c0 < nchunks; c0 += epoch) {
    const int64_t c1 = nchunks - c0 > epoch ? c0 + epoch : nchunks;
    for (int64_t chunk = c0; chunk < c1; chunk += gridDim.x) {
        // One 64-bit division per chunk, a scalar one; R < 2^31, so what is left of a lane's index behind p_lo * R divides in 32 bits.
        const int64_t t0 = chunk << lanes_log2;
        const int64_t p_lo = t0 / R;
        const uint32_t rem0 = (uint32_t)(t0 - p_lo * R);
        const int64_t left = total - 1 - t0;
        const uint32_t last_lane = left < lanes - 1 ? (uint32_t)left : (uint32_t)(lanes - 1);      // the chunk's last lane with work
        const int32_t np_chunk = (int32_t)((rem0 + last_lane) / (uint32_t)R) + 1;                 // rows its lanes touch
        for (int32_t pl = __builtin_amdgcn_readfirstlane(wave); pl < np_chunk; pl += nwaves) {   // the wave index is uniform: say so
            uint8_t* rb = reinterpret_cast<uint8_t*>(rows + pl * 3 * N4);
            const bool bad = resample_encode(a, p_lo + pl, rb, meta + 2 * pl, scr + 64 * wave, lane);
            const bool neg = shortest_rank_row(a.tokens + (p_lo + pl) * (int64_t)N, N, (lds_u8*)(rb + 4 * N4), (lds_u8*)(rb + 8 * N4));
            if (__ballot(bad) && lane == 0) atomicOr(shortest_args_again()->err_flag, 1u);               // the error bits are raised where they are found: no lane carries them
            if (__ballot(neg) && lane == 0) atomicOr(shortest_args_again()->err_flag, 16u);
        }
        __syncthreads();
        const bool live = (uint32_t)tid <= last_lane;                                // a lane past the end walks with the last one and emits nothing
        const uint32_t off = rem0 + (live ? (uint32_t)tid : last_lane);
        const int32_t row = (int32_t)(off / (uint32_t)R);
        const int32_t rr = SHUF ? (int32_t)(off - (uint32_t)row * (uint32_t)R) : 0;
        const int64_t p = p_lo + row;
        const int32_t tcode = meta[2 * row];
        if (SHUF) for (int w = 0; w < N4; ++w) arr[(w << lanes_log2) + tid] = 0x03020100u + 0x04040404u * (uint32_t)w;
        for (int w = 0; w < NW; ++w) bits[(w << lanes_log2) + tid] = 0u;
        const uint8_t* my_row = rows_b + (int64_t)row * 3 * N4 * 4;                 // codes
        const uint8_t* my_trank = my_row + 4 * N4;
        const uint8_t* my_by_rank = my_row + 8 * N4;
        const int32_t* tok_lo = a.tokens + p_lo * (int64_t)N;                       // uniform: the lane's tokens are tok_lo[row * N + idx]
        const uint32_t tok_at = (uint32_t)row * (uint32_t)N;
        uint64_t arg = 0;
        if (SHUF) {
            kernarg_args* ka = shortest_args_again();
            const uint64_t s = mix64((ka->seed ^ kResampleSalt) + kGolden * (uint64_t)(ka->p_offset + p + 1));
            arg = s + kGolden * ((uint64_t)(uint32_t)(ka->r_begin + rr) * (uint64_t)N + 1ull);
        }
        // the state of one walk over the kept samples of a boundary
        uint32_t maxc = 0, nmodes = 0, tc = 0, min_x = 0;                         // min_x (pool order): a sample of the smallest modal value
        long long voted = 0;
        int32_t last = 0;
        // budget ord[q], k launched and m kept, from the walk's state (every lane of the wave is here: q, k and m are uniform)
        auto emit = [&](int q, int32_t k, int32_t m) {
            const int32_t b = __builtin_amdgcn_readfirstlane(ord[q]);
            const bool hit = live && tcode >= 0 && maxc != 0u && tc == maxc;
            const long long spent = voted + (long long)(k - m) * last;
            const uint32_t tcs = wave_sum_u32(live ? tc : 0u);
            const long long vs = wave_sum_i64(live ? voted : 0ll);
            const long long ss = wave_sum_i64(live ? spent : 0ll);
            const long long ls = wave_sum_i64(live ? (long long)last : 0ll);
            const unsigned long long ones = __ballot(hit && nmodes == 1u);
            if (lane == 0) {
                if (ones) atomicAdd(&tie[b * TC + 1], (uint32_t)__popcll(ones));
                if (tcs) atomicAdd(&acc[b], (unsigned long long)tcs);
                if (vs) atomicAdd(&acc[B + b], (unsigned long long)vs);
                if (ss) atomicAdd(&acc[2 * B + b], (unsigned long long)ss);
                if (ls) atomicAdd(&acc[3 * B + b], (unsigned long long)ls);
            }
            if (hit && nmodes != 1u) atomicAdd(&tie[b * TC + nmodes], 1u);
            if (__ballot(hit)) {                                                      // (uniform: the argument block is read by the wave)
                kernarg_args* ka = shortest_args_again();
                unsigned long long* per = ka->per_resample;
                if (hit && per) {
                    if (nmodes < (uint32_t)ka->M) atomicAdd(&per[((int64_t)rr * B + b) * ka->M + nmodes], 1ull);
                    else atomicOr(ka->err_flag, 2u);
                }
            }
            if (!SHUF) {
                kernarg_args* ka = shortest_args_again();
                scv_cell* cells_out = ka->cells_out;
                int64_t* cell_tokens_out = ka->cell_tokens_out;
                const int64_t cell = (p_lo + row) * (int64_t)B + b;
                if (live && cells_out) {
                    int32_t mm = -1;
                    if (maxc) mm = resample_min_mode(*(const ResampleArgs*)ka, p_lo + row, min_x, (uint32_t)my_row[min_x]);
                    uint32_t* cw = reinterpret_cast<uint32_t*>(cells_out) + 4 * cell;      // scv_cell: 4-byte aligned only
                    cw[0] = maxc;
                    cw[1] = tc;
                    cw[2] = nmodes | ((uint32_t)(uint16_t)(int16_t)mm << 16);
                    cw[3] = hit ? 1u : 0u;
                }
                if (live && cell_tokens_out) cell_tokens_out[cell] = spent;
            }
        };
        if (!SHUF) for (int q = 0; q < q0; ++q) emit(q, 0, 0);                       // k = 0: the empty cells of the pool order
        int q = q0;
        int32_t next_k = q < B ? __builtin_amdgcn_readfirstlane(ks[q]) : 0x7fffffff;
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
            const uint32_t r = (uint32_t)my_trank[x];
            bits[((r >> 5) << lanes_log2) + tid] |= 1u << (r & 31u);
            if (i + 1 == next_k) {
                const int32_t distinct = meta[2 * row + 1];
                for (int w = 0; w < ((distinct + 3) >> 2); ++w) cnt[(w << lanes_log2) + tid] = 0u;
                maxc = 0; nmodes = 0; tc = 0; min_x = 0; voted = 0; last = 0;
                int wi = 0, taken = 0;
                uint32_t cur = bits[tid];
                do {                                                                  // every budget of this k, in ascending m
                    const int32_t m = __builtin_amdgcn_readfirstlane(ms[q]);
                    for (; taken < m; ++taken) {                                      // k >= m bits are set: the skip ends on a set bit
                        while (cur == 0u && wi < NW - 1) { ++wi; cur = bits[(wi << lanes_log2) + tid]; }
                        const uint32_t rk = ((uint32_t)wi << 5) + (uint32_t)(__ffs((int)cur) - 1);
                        cur &= cur - 1u;
                        uint32_t idx = (uint32_t)my_by_rank[rk & 255u];
                        idx = idx < (uint32_t)N ? idx : (uint32_t)N - 1u;             // (a rank is below N: idx is a pool index)
                        const uint32_t code = (uint32_t)my_row[idx];
                        const uint32_t ac = resample_byte(code, lanes_log2, lane_byte);
                        const uint32_t c = (uint32_t)cnt_b[ac] + 1u;
                        cnt_b[ac] = (uint8_t)c;
                        if (c > maxc) { maxc = c; nmodes = 1u; if (!SHUF) min_x = idx; }
                        else if (c == maxc) { nmodes += 1u; if (!SHUF && code < (uint32_t)my_row[min_x]) min_x = idx; }
                        tc += (int32_t)code == tcode ? 1u : 0u;
                        last = tok_lo[tok_at + idx];
                        voted += (long long)last;
                    }
                    emit(q, i + 1, m);
                    ++q;
                    next_k = q < B ? __builtin_amdgcn_readfirstlane(ks[q]) : 0x7fffffff;
                } while (next_k == i + 1);
            }
        }
        __syncthreads();                                                              // the rows are rewritten by the next chunk
    }
    if (c1 < nchunks) {                                                               // another epoch follows (uniform)
        for (int i = tid; i < B * TC; i += lanes) {
            const uint32_t v = tie[i];
            if (v) { atomicAdd(&shortest_args_again()->tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v); tie[i] = 0u; }
        }
        __syncthreads();
    }
    }
    __syncthreads();
    kernarg_args* ka = shortest_args_again();
    unsigned long long* tie_hits = ka->tie_hits;
    for (int i = tid; i < B * TC; i += lanes) {
        const uint32_t v = tie[i];
        if (v) atomicAdd(&tie_hits[(int64_t)(i / TC) * SCV_TIE_CLASSES + (i % TC)], (unsigned long long)v);
    }
    if (tid < B) {
        if (ka->truth_sum && acc[tid]) atomicAdd(&ka->truth_sum[tid], acc[tid]);
        if (ka->token_sum && acc[B + tid]) atomicAdd(&ka->token_sum[tid], acc[B + tid]);
        if (ka->spent_sum && acc[2 * B + tid]) atomicAdd(&ka->spent_sum[tid], acc[2 * B + tid]);
        if (ka->latency_sum && acc[3 * B + tid]) atomicAdd(&ka->latency_sum[tid], acc[3 * B + tid]);
    }
}

__device__ __forceinline__ void shortest_body(const ResampleArgs& a, uint32_t* smem) {
    if (a.order == kOrderShuffled) shortest_run<true>(a, smem);
    else shortest_run<false>(a, smem);
}

}  // namespace scv
