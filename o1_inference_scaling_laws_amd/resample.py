"""CPU mirror (numpy, uint64) of scv_resample_prefix_i32, spec in include/scvote.h: the expected majority vote over random
orderings of each problem's sample pool.  Vectorised over the (problem, resample) lanes, one loop iteration per Fisher-Yates
step; the same role as synth.py -- the executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .scoring import accuracy_from_tie_classes, avg_tokens_used, exact_accuracy_from_tie_classes
from .synth import G, _MASK32, mix64

NUM_BINS, TIE_CLASSES = 1024, 1025
SEED_SALT = np.uint64(0xD6E8FEB86659FD93)
MAX_N, MAX_B = 256, 32
ERR_DOMAIN_BIT, ERR_CLASS_BIT = 1, 2           # bits of the device error word (include/scvote.h)


def problem_streams(seed: int, pg) -> np.ndarray:
    """s_p = mix64((seed ^ 0xD6E8FEB86659FD93) + G * (pg + 1)) for global problem indices pg."""
    pg = np.asarray(pg, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64((np.uint64(seed) ^ SEED_SALT) + G * (pg + np.uint64(1)))


def swap_index(s, r, i: int, N: int):
    """j of Fisher-Yates step i of resample r: i + mulhi32(hi32(mix64(s + G * (r * N + i + 1))), N - i)."""
    with np.errstate(over="ignore"):
        u = mix64(np.asarray(s, dtype=np.uint64) + G * (np.asarray(r, dtype=np.uint64) * np.uint64(N) + np.uint64(i + 1)))
    return np.uint64(i) + (((u >> np.uint64(32)) & _MASK32) * np.uint64(N - i) >> np.uint64(32))


@dataclass
class ResampleResult:
    """Integer outputs of one resampled-majority call + the floats derived from them.  Every denominator is
    P * R (cells per budget): accuracy(b) is the expected maj@k_b over orderings, averaged over problems."""
    P: int
    R: int
    tie_class_hits: np.ndarray          # int64 [B, 1025]
    token_sum: np.ndarray               # int64 [B]
    truth_count_sum: np.ndarray         # int64 [B]
    per_resample: np.ndarray | None     # int64 [R, B, M]: class counts of each ordering, summed over problems
    error_bits: int = 0                 # bit 0: a vote outside 0..1023; bit 1: a hit with n_modes >= M

    def _den(self):
        return self.P * self.R

    def accuracy(self, b: int = 0) -> float:
        return accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def exact_accuracy(self, b: int = 0):
        return exact_accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def avg_tokens_used(self, b: int = 0) -> np.float64:
        return avg_tokens_used(self.token_sum[b], self._den())

    def resample_accuracy(self, b: int = 0) -> np.ndarray:
        """accuracy of every single ordering r (its spread is the noise of a one-ordering curve): float64 [R]."""
        if self.per_resample is None:
            raise ValueError("per_resample was not requested")
        m = np.arange(1, self.per_resample.shape[2], dtype=np.float64)
        return (self.per_resample[:, b, 1:] / m).sum(axis=1) / self.P


def dense_codes(pool: np.ndarray, open_domain: bool = False):
    """Votes outside 0..1023 -> bin 1023 (and a flag); then each row re-encoded to value-ordered dense codes.
    Returns (codes int64 [P, N], distinct values per row [P], sorted distinct values per row (list), domain flag).
    ``open_domain`` (SCV_FLAG_OPEN_DOMAIN): every int32 is a value of its own, in signed order -- no clamp, never a domain flag."""
    v = np.asarray(pool, dtype=np.int64)
    if open_domain:
        v = np.asarray(pool).astype(np.int32).astype(np.int64)
        bad = np.zeros(v.shape, dtype=bool)
    else:
        bad = (v < 0) | (v >= NUM_BINS)
    v = np.where(bad, NUM_BINS - 1, v)
    codes = np.empty_like(v)
    uniq = []
    for p in range(v.shape[0]):
        u, inv = np.unique(v[p], return_inverse=True)
        codes[p] = inv.reshape(-1)
        uniq.append(u)
    return codes, uniq, bool(bad.any())


def truth_codes(uniq, truth, open_domain: bool = False) -> np.ndarray:
    """The truth's code in its row (``uniq``: the rows' sorted distinct values, from dense_codes), or -1: absent, or -- without
    ``open_domain`` -- outside the bins (such a truth never hits)."""
    tcode = np.full(len(uniq), -1, dtype=np.int64)
    for p, u in enumerate(uniq):
        t = int(truth[p])
        if open_domain or 0 <= t < NUM_BINS:
            k = np.searchsorted(u, t)
            if k < len(u) and u[k] == t:
                tcode[p] = k
    return tcode


def resample_prefix(pool, truth, n_valid, r_begin: int, r_end: int, seed: int, tokens=None, p_offset: int = 0,
                    M: int | None = None, open_domain: bool = False) -> ResampleResult:
    """pool int32 [P, N], truth int32 [P], n_valid int32 [B] (budget b votes over the first clamp(n_valid[b], 0, N) of a
    random ordering), resamples [r_begin, r_end).  ``M``: per_resample classes (None: not computed)."""
    pool = np.asarray(pool)
    if pool.ndim != 2:
        raise ValueError("pool must be [P, N]")
    P, N = pool.shape
    truth = np.asarray(truth, dtype=np.int64)
    nv = np.asarray(n_valid, dtype=np.int64).reshape(-1)
    B = nv.shape[0]
    if not (1 <= N <= MAX_N and 1 <= B <= MAX_B and 0 <= r_begin <= r_end < 2 ** 31) or truth.shape != (P,):
        raise ValueError(f"bad shape P={P} N={N} B={B} r=[{r_begin},{r_end})")
    if M is not None and M < 1:
        raise ValueError("M must be >= 1")
    R = r_end - r_begin
    ks = np.clip(nv, 0, N)
    tie = np.zeros((B, TIE_CLASSES), dtype=np.int64)
    tsum = np.zeros(B, dtype=np.int64)
    tcsum = np.zeros(B, dtype=np.int64)
    per = np.zeros((R, B, M), dtype=np.int64) if M is not None else None
    codes, uniq, bad = dense_codes(pool, open_domain)
    err = ERR_DOMAIN_BIT if bad else 0
    L = P * R
    if L == 0:
        return ResampleResult(P, R, tie, tsum, tcsum, per, err)
    tcode = truth_codes(uniq, truth, open_domain)
    lp = np.repeat(np.arange(P), R)                                  # lanes problem-major
    lr = np.tile(np.arange(r_begin, r_end, dtype=np.int64), P)
    s = problem_streams(seed, p_offset + lp)
    perm = np.tile(np.arange(N, dtype=np.int16), (L, 1))
    cnt = np.zeros((L, N), dtype=np.int32)
    maxc = np.zeros(L, dtype=np.int32)
    nmodes = np.zeros(L, dtype=np.int32)
    tc = np.zeros(L, dtype=np.int64)
    tok = np.zeros(L, dtype=np.int64)
    tok_rows = None if tokens is None else np.asarray(tokens, dtype=np.int64)
    lanes = np.arange(L)
    order = np.argsort(ks, kind="stable")
    kmax = int(ks.max())
    q = 0
    while q < B and ks[order[q]] == 0:                               # empty subsets: no hit, nothing to add
        q += 1
    for i in range(kmax):
        j = swap_index(s, lr.astype(np.uint64), i, N).astype(np.int64)
        x = perm[lanes, j].astype(np.int64)
        perm[lanes, j] = perm[:, i]
        perm[:, i] = x
        code = codes[lp, x]
        c = cnt[lanes, code] + 1
        cnt[lanes, code] = c
        gt, eq = c > maxc, c == maxc
        nmodes = np.where(gt, 1, np.where(eq, nmodes + 1, nmodes))
        maxc = np.where(gt, c, maxc)
        tc += code == tcode[lp]
        if tok_rows is not None:
            tok += tok_rows[lp, x]
        while q < B and ks[order[q]] == i + 1:
            b = int(order[q])
            hit = (tcode[lp] >= 0) & (tc == maxc)
            tie[b] += np.bincount(nmodes[hit], minlength=TIE_CLASSES)[:TIE_CLASSES]
            tcsum[b] += int(tc.sum())
            tsum[b] += int(tok.sum())
            if per is not None:
                m = nmodes[hit]
                if (m >= M).any():
                    err |= ERR_CLASS_BIT
                keep = m < M
                per[:, b, :] += np.bincount((lr[hit] - r_begin)[keep] * M + m[keep], minlength=R * M).reshape(R, M)
            q += 1
    return ResampleResult(P, R, tie, tsum, tcsum, per, err)
