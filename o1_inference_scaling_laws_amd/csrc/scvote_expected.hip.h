// scvote_expected.hip.h -- the exact expected majority vote over all k-subsets of a pool (scv_expected_majority_i32): the second body of
// scv_resample_prefix<false> (ResampleArgs::mode == kResampleModeExpected), included by scvote_resample.hip.h.
//
// The prefix of a uniformly random ordering is a uniformly random k-subset, so the R -> infinity limit of scv_resample_prefix has a closed
// form (include/scvote.h): with c_t truth votes and c_v votes of every other value v,
//   E_k = C(N,k)^-1 sum_{j=1..min(c_t,k)} C(c_t,j) sum_u A_j(k-j,u) / (1+u),   H_k the same without the 1 / (1+u)
//   A_j(s,u) = [x^s y^u] prod_{v != t} ( sum_{i < min(c_v+1, j)} C(c_v,i) x^i + [c_v >= j] C(c_v,j) x^j y ).
// sum_u A(s,u) / (1+u) = integral_0^1 A(s,y) dy, and A_j(s, .) has degree <= U_j = min(#{v != t : c_v >= j}, (k_max - j) / j) in y, so
// Gauss-Legendre with Q_j = ceil((U_j + 1) / 2) points on [0, 1] is exact.  Each (j, point) is then a product of polynomials in x alone.
//
// How:
//  * one workgroup of kExpectedLanes lanes per problem (persistent grid).  Wave 0 encodes the row (resample_encode_row: value-ordered byte
//    codes, the truth's code); the workgroup counts votes per code and classes per count (hist[c], LDS integer atomics: exact, order-free).
//  * work items, numbered in a fixed order and dealt round-robin to the waves:
//      j = 1:     one item, y = 1: prod (1 + c_v x) = e_s(c), and A_1(s,u) = e_s [u = s], so E takes vec[k-1] / k and H vec[k-1].
//      2 <= j <= min(c_t, max_{v != t} c_v, k_max): Q_j quadrature items (node y_q, weight w_q) and one at y = 1 for H (numbered even
//                 when hit_out is NULL and then skipped, so that the score's summation order is the same with or without H).
//    Classes with c_v < j only contribute (1 + x)^{c_v}: all of them fold into the start vector C(L_j, s), L_j their vote total.  The
//    classes with c_v >= j are multiplied in one factor at a time, hist[c] times the factor of count c.
//    j > max_{v != t} c_v: no class can tie, A_j(s, 0) = C(N - c_t, s) -- summed directly in the epilogue, no item.
//  * an item's vector (256 doubles, 4 consecutive coefficients per lane) lives in the wave's LDS, one pad double per 32 so that the lanes'
//    reads (stride 4 doubles) spread over the banks.  A factor of degree j costs j + 1 steps; a step is one tap (its lane's register read
//    back with readlane; tap 0 is 1), one LDS read (the window slides by one coefficient) and 4 FMAs.
//  * lanes b < B of each wave add the item's term C(c_t,j) w_q vec[k_b - j] to the wave's own LDS sums in item order; the waves' sums are added
//    in wave order, then the closed-form tail, then one division by C(N,k) and one store per (p, b).  Nothing depends on the problem's
//    position in the call or on the grid: whole calls, shards, HOST and DEVICE mode give the same bits.
// Every term is a nonnegative count of subsets (<= 2^256) times nonnegative weights: no subtraction, so no cancellation, and a rational 0
// comes out as exactly 0.0.  Binomials and Gauss-Legendre points come from the context's table (scv_create).  No scratch, no allocation.
#pragma once

namespace scv {

__device__ __forceinline__ int expected_slot(int e) { return e + (e >> 5); }                  // e >= -129: >= -kExpectedZeros

__device__ __forceinline__ void expected_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double expected_readlane(double v, int i) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), i);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// one wave: vec <- vec * f^m, f = sum_{i < j} C(c,i) x^i + y C(c,j) x^j (c >= j), coefficients 0 .. 255; binom_c = the row C(c, .).
// Tap 0 is C(c,0) = 1; taps 1 .. j (j <= 128) sit in lane i - 1 of tap_lo (i <= 64) or lane i - 65 of tap_hi.
__device__ __forceinline__ void expected_mul(double* vec, const double* binom_c, int j, double y, int m, int lane) {
    double tap_lo = lane < j ? binom_c[lane + 1] : 0.0;
    double tap_hi = lane + 64 < j ? binom_c[lane + 65] : 0.0;
    if (lane + 1 == j) tap_lo *= y;
    if (lane + 65 == j) tap_hi *= y;
    const int s0 = 4 * lane;
    for (int rep = 0; rep < m; ++rep) {
        double o0 = vec[expected_slot(s0)], o1 = vec[expected_slot(s0 + 1)], o2 = vec[expected_slot(s0 + 2)], o3 = vec[expected_slot(s0 + 3)];
        double w0 = vec[expected_slot(s0 - 1)], w1 = o0, w2 = o1, w3 = o2;          // tap 0 done; window w_r = vec[s0 + r - 1]
#pragma nounroll
        for (int i = 1; i <= j; ++i) {                                               // window w_r = vec[s0 + r - i]
            const double t = expected_readlane(i <= 64 ? tap_lo : tap_hi, (i - 1) & 63);
            o0 = __fma_rn(t, w0, o0);
            o1 = __fma_rn(t, w1, o1);
            o2 = __fma_rn(t, w2, o2);
            o3 = __fma_rn(t, w3, o3);
            w3 = w2; w2 = w1; w1 = w0;
            w0 = vec[expected_slot(s0 - i - 1)];                                     // zeros below coefficient 0
        }
        expected_wave_sync();
        vec[expected_slot(s0)] = o0; vec[expected_slot(s0 + 1)] = o1; vec[expected_slot(s0 + 2)] = o2; vec[expected_slot(s0 + 3)] = o3;
        expected_wave_sync();
    }
}

__device__ __forceinline__ int expected_budget(const ResampleArgs& a, int b) {
    const int32_t k = a.n_valid[b];
    return k < 0 ? 0 : (k > a.N ? a.N : k);
}

__device__ __forceinline__ void expected_majority_body(const ResampleArgs& a, uint32_t* smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
    const int N = a.N, B = a.B;
    double* vecs = reinterpret_cast<double*>(smem);                                  // [nw][kExpectedZeros + kExpectedVec]
    double* sums = vecs + nw * (kExpectedZeros + kExpectedVec);                                       // [2][nw][32]
    int32_t* cnt = reinterpret_cast<int32_t*>(sums + 2 * nw * 32);                   // [256]
    int32_t* hist = cnt + 256;                                                       // [260]
    int32_t* meta = hist + 260;                                                      // [4]
    uint32_t* codes = reinterpret_cast<uint32_t*>(meta + 4);                         // [64]
    uint32_t* scr = codes + 64;                                                      // [64]
    double* vec = vecs + wave * (kExpectedZeros + kExpectedVec) + kExpectedZeros;
    for (int i = lane; i < kExpectedZeros; i += 64) vec[i - kExpectedZeros] = 0.0;
    const double* binom = a.tab;
    const double* gl = a.tab + kExpectedBinomWords;
    int kmax = 0;
    for (int b = 0; b < B; ++b) kmax = max(kmax, expected_budget(a, b));
    const int kb = lane < B ? expected_budget(a, lane) : 0;                          // lanes b < B of every wave: budget b
    bool bad = false;
    for (int64_t p = blockIdx.x; p < a.P; p += gridDim.x) {
        for (int i = tid; i < 256 + 260; i += (int)blockDim.x) cnt[i] = 0;          // cnt | hist
        if (wave == 0) bad |= resample_encode(a, p, reinterpret_cast<uint8_t*>(codes), meta, scr, lane);
        __syncthreads();
        const uint8_t* cb = reinterpret_cast<const uint8_t*>(codes);
        for (int e = tid; e < N; e += (int)blockDim.x) atomicAdd(&cnt[cb[e]], 1);
        __syncthreads();
        const int tcode = __builtin_amdgcn_readfirstlane(meta[0]), distinct = __builtin_amdgcn_readfirstlane(meta[1]);
        const int ct = tcode >= 0 ? __builtin_amdgcn_readfirstlane(cnt[tcode]) : 0;
        if (tid < distinct && tid != tcode) {
            atomicAdd(&hist[cnt[tid]], 1);
            atomicMax(&hist[257], cnt[tid]);
        }
        __syncthreads();
        const int mo = __builtin_amdgcn_readfirstlane(hist[257]);                                                   // the largest count of another value
        const int jmax = min(min(ct, mo), kmax);
        double* acc_e = sums + wave * 32;                                            // this wave's E and H sums, lanes b < B, in item order
        double* acc_h = sums + (nw + wave) * 32;
        if (lane < 32) { acc_e[lane] = 0.0; acc_h[lane] = 0.0; }
        int item = 0;
        int G = distinct - (tcode >= 0 ? 1 : 0), S = N - ct;                        // classes v != t with c_v >= j, their votes
        for (int j = 1; j <= jmax; ++j) {
            if (j >= 2) {
                const int h = __builtin_amdgcn_readfirstlane(hist[j - 1]);
                G -= h;
                S -= (j - 1) * h;
            }
            const int L = N - ct - S;
            const int Q = j == 1 ? 0 : (min(G, (kmax - j) / j) + 2) / 2;
            const int nitems = j == 1 ? 1 : Q + 1;
            const double cj = binom[ct * (ct + 1) / 2 + j];
            for (int q = 0; q < nitems; ++q, ++item) {
                const bool at_one = q == Q;                                          // y = 1: j = 1, or the H item
                if (item % nw != wave || (j >= 2 && at_one && !a.hit_out)) continue;  // (numbered either way: E's order does not depend on H)
                const double y = at_one ? 1.0 : gl[Q * (Q - 1) + 2 * q];
                const double w = at_one ? 1.0 : gl[Q * (Q - 1) + 2 * q + 1];
#pragma nounroll
                for (int s = lane; s < 256; s += 64) vec[expected_slot(s)] = s <= L ? binom[L * (L + 1) / 2 + s] : 0.0;
                expected_wave_sync();
                for (int c = j; c <= mo; ++c) {
                    const int m = __builtin_amdgcn_readfirstlane(hist[c]);
                    if (m) expected_mul(vec, binom + c * (c + 1) / 2, j, y, m, lane);
                }
                if (kb >= j) {
                    const double v = vec[expected_slot(kb - j)];
                    if (j == 1) { acc_e[lane] += (double)ct * v / (double)kb; acc_h[lane] += (double)ct * v; }
                    else if (at_one) acc_h[lane] += cj * v;
                    else acc_e[lane] += cj * w * v;
                }
                expected_wave_sync();
            }
        }
        __syncthreads();
        if (tid < B) {
            const int k = expected_budget(a, tid);
            double e = 0.0, h = 0.0;
            for (int w = 0; w < nw; ++w) { e += sums[w * 32 + tid]; h += sums[(nw + w) * 32 + tid]; }
            double tail = 0.0;                                                       // j > mo: no tie, C(c_t, j) C(N - c_t, k - j)
            const int rest = N - ct;
            for (int j = max(max(mo + 1, 1), k - rest); j <= min(ct, k); ++j)
                tail += binom[ct * (ct + 1) / 2 + j] * binom[rest * (rest + 1) / 2 + (k - j)];
            const double den = binom[N * (N + 1) / 2 + k];
            a.score_out[p * B + tid] = k == 0 ? 0.0 : (e + tail) / den;
            if (a.hit_out) a.hit_out[p * B + tid] = k == 0 ? 0.0 : (h + tail) / den;
        }
        __syncthreads();                                                             // LDS is rewritten by the next problem
    }
    if (__ballot(bad) && lane == 0) atomicOr(a.err_flag, 1u);
}

}  // namespace scv
