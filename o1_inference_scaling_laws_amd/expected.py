"""CPU statement of scv_expected_majority_i32 (spec in include/scvote.h): the exact expected majority vote over all k-subsets of each
problem's pool -- the limit of resample.py's shuffles as R grows without bound.  The same role as resample.py for the resample kernel:

* ``expected_majority_exact`` -- the rationals E and H (fractions.Fraction [P][B]) from the subset-counting formula, with Python
  integers in the DP over (s, u) and rationals only at the end.  It uses the small-class fold and the no-tie closed form, and the
  e_s recurrence for j = 1, so N = 256 stays in seconds.
* ``expected_majority_quadrature`` -- the GPU's algorithm in numpy float64: the same work items (j, Gauss-Legendre point), the same
  identities, the kernel's own Gauss-Legendre rules (``_gl01``).  The tests pin it to the rationals; it is where the kernel's bookkeeping was
  rehearsed.
* ``ExpectedResult`` -- what Engine.expected_majority returns."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

NUM_BINS = 1024
MAX_N, MAX_B = 256, 32


@dataclass
class ExpectedResult:
    """Per-problem expected scores of one call.  score / hit_prob float64 [P, B] (hit_prob None when not requested); ks the budgets
    clamp(n_valid, 0, N); token_total the sum of every vote's tokens over the P x N pool (None without tokens)."""
    score: np.ndarray
    hit_prob: np.ndarray | None
    ks: np.ndarray
    N: int
    token_total: int | None = None

    @property
    def P(self) -> int:
        return int(self.score.shape[0])

    def accuracy(self, b: int = 0) -> float:
        """Expected maj@k_b averaged over problems (a fixed-order exact-rounding sum, then / P)."""
        return math.fsum(self.score[:, b].tolist()) / self.P if self.P else 0.0

    def hit_rate(self, b: int = 0) -> float:
        """Probability that the truth is among the modes, averaged over problems."""
        if self.hit_prob is None:
            raise ValueError("hit_prob was not requested")
        return math.fsum(self.hit_prob[:, b].tolist()) / self.P if self.P else 0.0

    def avg_tokens_used(self, b: int = 0) -> float:
        """Expected tokens of a k_b-subset, averaged over problems: k_b * sum(tokens) / (N * P), rounded once from the exact rational."""
        if self.token_total is None or self.P == 0:
            return 0.0
        return float(Fraction(int(self.ks[b]) * self.token_total, self.N * self.P))


def _check(pool, truth, n_valid):
    pool = np.asarray(pool, dtype=np.int64)
    if pool.ndim != 2:
        raise ValueError("pool must be [P, N]")
    P, N = pool.shape
    truth = np.asarray(truth, dtype=np.int64).reshape(-1)
    nv = np.asarray(n_valid, dtype=np.int64).reshape(-1)
    if not (1 <= N <= MAX_N and 1 <= nv.shape[0] <= MAX_B) or truth.shape != (P,):
        raise ValueError(f"bad shape P={P} N={N} B={nv.shape[0]}")
    return pool, truth, np.clip(nv, 0, N), N


def row_classes(row, truth: int, open_domain: bool = False):
    """(c_t, [c_v for v != t]) of one pool row: votes outside 0..1023 count as 1023; a truth outside the bins has c_t = 0 and every
    value is an 'other' class.  ``open_domain`` (SCV_FLAG_OPEN_DOMAIN): every integer is a value of its own, the truth included."""
    v = np.asarray(row, dtype=np.int64)
    if not open_domain:
        v = np.where((v < 0) | (v >= NUM_BINS), NUM_BINS - 1, v)
    vals, counts = np.unique(v, return_counts=True)
    ct = 0
    others = []
    for x, c in zip(vals.tolist(), counts.tolist()):
        if x == truth and (open_domain or 0 <= truth < NUM_BINS):
            ct = c
        else:
            others.append(c)
    return ct, others


def domain_error(pool, open_domain: bool = False) -> bool:
    """Error bit 0 of the call: a vote outside 0..1023 (never under ``open_domain``)."""
    if open_domain:
        return False
    v = np.asarray(pool, dtype=np.int64)
    return bool(((v < 0) | (v >= NUM_BINS)).any())


def _no_tie_tail(N: int, ct: int, mo: int, k: int) -> int:
    """sum over max(mo, 0) < j <= min(c_t, k) of C(c_t, j) C(N - c_t, k - j): subsets in which no other value can reach the truth's j."""
    return sum(math.comb(ct, j) * math.comb(N - ct, k - j) for j in range(mo + 1, min(ct, k) + 1))


def _exact_row(N: int, ct: int, others, ks):
    kmax = int(max(ks))
    mo = max(others, default=0)
    num_e = [Fraction(0)] * len(ks)
    num_h = [0] * len(ks)
    jmax = min(ct, mo, kmax)
    if jmax >= 1:                                                  # j = 1: A_1(s, u) = e_s(c) [u = s]
        e = [1] + [0] * (kmax - 1)
        for c in others:
            for s in range(kmax - 1, 0, -1):
                e[s] += c * e[s - 1]
        for b, k in enumerate(ks):
            if k >= 1:
                num_e[b] += Fraction(ct * e[k - 1], k)
                num_h[b] += ct * e[k - 1]
    for j in range(2, jmax + 1):
        big = [c for c in others if c >= j]
        L = sum(c for c in others if c < j)                        # small classes: one binomial (1 + x)^L
        D = kmax - j
        U = min(len(big), D // j)
        A = np.zeros((D + 1, U + 1), dtype=object)
        A[:, :] = 0
        for s in range(min(L, D) + 1):
            A[s, 0] = math.comb(L, s)
        for c in big:
            new = np.zeros_like(A)
            new[:, :] = 0
            for i in range(min(j - 1, D) + 1):
                new[i:, :] += math.comb(c, i) * A[:D + 1 - i, :]
            if D >= j and U >= 1:
                new[j:, 1:] += math.comb(c, j) * A[:D + 1 - j, :-1]
            A = new
        lcm = math.lcm(*range(1, U + 2))
        cj = math.comb(ct, j)
        for b, k in enumerate(ks):
            if k >= j:
                row = A[k - j]
                num_e[b] += Fraction(cj * sum(int(row[u]) * (lcm // (u + 1)) for u in range(U + 1)), lcm)
                num_h[b] += cj * sum(int(x) for x in row)
    E, H = [], []
    for b, k in enumerate(ks):
        k = int(k)
        if k == 0 or ct == 0:
            E.append(Fraction(0))
            H.append(Fraction(0))
            continue
        tail = _no_tie_tail(N, ct, mo, k)
        den = math.comb(N, k)
        E.append((num_e[b] + tail) / den)
        H.append(Fraction(num_h[b] + tail, den))
    return E, H


def expected_majority_exact(pool, truth, n_valid, open_domain: bool = False):
    """(E, H): lists [P][B] of fractions.Fraction -- the expected score (1 / n_modes on a hit) and the hit probability of the majority vote
    over a uniformly random k_b-subset of pool[p], k_b = clamp(n_valid[b], 0, N)."""
    pool, truth, ks, N = _check(pool, truth, n_valid)
    E, H = [], []
    for p in range(pool.shape[0]):
        ct, others = row_classes(pool[p], int(truth[p]), open_domain)
        e, h = _exact_row(N, ct, others, [int(k) for k in ks])
        E.append(e)
        H.append(h)
    return E, H


@functools.lru_cache(maxsize=None)
def _gl01(Q: int):
    """The kernel's Gauss-Legendre rule of Q points on [0, 1] (build_expected_table in csrc/scvote_expected_table.h, step for step):
    Newton on P_Q from x = -cos(pi (q + 3/4) / (Q + 1/2)) in np.longdouble -- the x86-64 C long double, so the same roundings and the
    same table bits (tests/test_expected_table.py).  numpy's leggauss weights are off by up to 2e-12 relative for Q >= 40.
    Returns (nodes ascending, weights), float64 [Q] each."""
    ld = np.longdouble
    one, pi = ld(1), ld("3.141592653589793238462643383279502884")
    ys, ws = np.empty(Q), np.empty(Q)

    def legendre(x):
        p0, p1 = one, x
        for n in range(2, Q + 1):
            p0, p1 = p1, (ld(2 * n - 1) * x * p1 - ld(n - 1) * p0) / ld(n)
        return p0, p1, ld(Q) * (x * p1 - p0) / (x * x - one)

    for q in range(Q):
        x = -np.cos(pi * (ld(q) + ld("0.75")) / (ld(Q) + ld("0.5")))
        for _ in range(30):
            _p0, p1, dp = legendre(x)
            dx = p1 / dp
            x = x - dx
            if abs(dx) < ld("1e-18"):
                break
        _p0, _p1, dp = legendre(x)
        ys[q] = np.float64((one + x) / ld(2))
        ws[q] = np.float64(one / ((one - x * x) * dp * dp))
    ys.flags.writeable = ws.flags.writeable = False
    return ys, ws


def work_items(N: int, ct: int, others, kmax: int, hit: bool = True):
    """The kernel's items of one problem, in its order: (j, y, w, kind) with kind 'j1' (y = 1, E takes vec[k-1] / k), 'quad' (a
    Gauss-Legendre point) or 'hit' (y = 1, H only); plus (L_j, [counts c >= j]) per item.  j runs over 1 .. min(c_t, max other, k_max)."""
    mo = max(others, default=0)
    items = []
    for j in range(1, min(ct, mo, kmax) + 1):
        big = sorted(c for c in others if c >= j)
        L = sum(c for c in others if c < j)
        if j == 1:
            items.append((1, 1.0, 1.0, "j1", L, big))
            continue
        U = min(len(big), (kmax - j) // j)
        Q = (U + 2) // 2
        ys, ws = _gl01(Q)
        items += [(j, float(y), float(w), "quad", L, big) for y, w in zip(ys, ws)]
        if hit:
            items.append((j, 1.0, 1.0, "hit", L, big))
    return items


def item_fp64_ops(N: int, ct: int, others, kmax: int, hit: bool = True) -> int:
    """FP64 operations the kernel spends on one problem: 2 per FMA, 4 FMAs per lane and step over 64 lanes, (j + 1) steps per factor."""
    return sum(2 * 256 * (j + 1) * len(big) for j, _y, _w, _kind, _L, big in work_items(N, ct, others, kmax, hit))


def expected_majority_quadrature(pool, truth, n_valid, hit: bool = True, open_domain: bool = False):
    """The GPU's algorithm in numpy float64: (score [P, B], hit_prob [P, B] or None)."""
    pool, truth, ks, N = _check(pool, truth, n_valid)
    P, B = pool.shape[0], ks.shape[0]
    kmax = int(ks.max())
    score = np.zeros((P, B))
    hitp = np.zeros((P, B)) if hit else None
    for p in range(P):
        ct, others = row_classes(pool[p], int(truth[p]), open_domain)
        mo = max(others, default=0)
        acc_e = np.zeros(B)
        acc_h = np.zeros(B)
        for j, y, w, kind, L, big in work_items(N, ct, others, kmax, hit):
            D = kmax - j
            vec = np.array([float(math.comb(L, s)) if s <= L else 0.0 for s in range(D + 1)])
            for c in big:
                taps = np.array([float(math.comb(c, i)) for i in range(j)] + [float(math.comb(c, j)) * y])
                vec = np.convolve(vec, taps)[:D + 1]
            for b, k in enumerate(ks.tolist()):
                if k < j:
                    continue
                v = vec[k - j]
                if kind == "j1":
                    acc_e[b] += ct * v / k
                    acc_h[b] += ct * v
                elif kind == "hit":
                    acc_h[b] += math.comb(ct, j) * v
                else:
                    acc_e[b] += float(math.comb(ct, j)) * w * v
        for b, k in enumerate(ks.tolist()):
            if k == 0:
                continue
            tail = float(sum(float(math.comb(ct, j)) * float(math.comb(N - ct, k - j))
                             for j in range(max(mo + 1, 1, k - (N - ct)), min(ct, k) + 1)))
            den = float(math.comb(N, k))
            score[p, b] = (acc_e[b] + tail) / den
            if hit:
                hitp[p, b] = (acc_h[b] + tail) / den
    return score, hitp
