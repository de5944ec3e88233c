// scvote_expected_table.h -- the table of scv_expected_majority_i32 (binomials and Gauss-Legendre rules), built on the host at scv_create.
// Plain C++17 (no HIP): included by csrc/scvote_dispatch.h for the library and by tests/expected_table_check.cpp, which dumps it on the CPU
// for tests/test_expected_table.py (exactness of every rule on monomials, the binomials against exact integers, the CPU mirror's rules).
#pragma once

#include <cmath>
#include <vector>

namespace scv {

// the context's table: C(n, i) at n (n + 1) / 2 + i (0 <= i <= n <= 256), then for Q = 1 .. 64 Gauss-Legendre points on [0, 1],
// (node, weight) pairs of rule Q at kExpectedBinomWords + Q (Q - 1) + 2 q
constexpr int kExpectedMaxQ = 64;
constexpr int kExpectedBinomWords = 257 * 258 / 2;
constexpr int kExpectedTabWords = kExpectedBinomWords + kExpectedMaxQ * (kExpectedMaxQ + 1);

// The table (kExpectedTabWords doubles): C(n, i) for n <= 256 by Pascal's rule (every entry a sum of two nonnegative terms: relative
// error <= n * 2^-53), then the Gauss-Legendre rules of 1 .. 64 points mapped to [0, 1] (Newton on P_Q in long double).
inline void build_expected_table(std::vector<double>& t) {
    t.assign(kExpectedTabWords, 0.0);
    for (int n = 0; n <= 256; ++n) {
        double* row = t.data() + n * (n + 1) / 2;
        const double* up = t.data() + (n - 1) * n / 2;
        row[0] = row[n] = 1.0;
        for (int i = 1; i < n; ++i) row[i] = up[i - 1] + up[i];
    }
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int Q = 1; Q <= kExpectedMaxQ; ++Q) {
        double* rule = t.data() + kExpectedBinomWords + Q * (Q - 1);
        for (int q = 0; q < Q; ++q) {
            long double x = -cosl(pi * (q + 0.75L) / (Q + 0.5L)), dp = 1.0L;      // ascending nodes
            for (int it = 0; it < 30; ++it) {
                long double p0 = 1.0L, p1 = x;
                for (int n = 2; n <= Q; ++n) { const long double p2 = ((2 * n - 1) * x * p1 - (n - 1) * p0) / n; p0 = p1; p1 = p2; }
                dp = Q * (x * p1 - p0) / (x * x - 1.0L);
                const long double dx = p1 / dp;
                x -= dx;
                if (fabsl(dx) < 1e-18L) break;
            }
            long double p0 = 1.0L, p1 = x;
            for (int n = 2; n <= Q; ++n) { const long double p2 = ((2 * n - 1) * x * p1 - (n - 1) * p0) / n; p0 = p1; p1 = p2; }
            dp = Q * (x * p1 - p0) / (x * x - 1.0L);
            rule[2 * q] = (double)((1.0L + x) / 2.0L);
            rule[2 * q + 1] = (double)(1.0L / ((1.0L - x * x) * dp * dp));          // 2 / ((1 - x^2) P'(x)^2), halved for [0, 1]
        }
    }
}

}  // namespace scv
