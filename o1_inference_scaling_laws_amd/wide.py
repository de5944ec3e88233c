"""CPU mirror (numpy, uint64) of scv_resample_wide_i32, spec in include/scvote.h: the expected majority vote over random orderings
of pools of up to 4096 samples.  An ordering is defined by sort keys, not by a Fisher-Yates walk: one np.argsort over the uint64 words of
every resample of a problem.  The same role as resample.py -- the executable statement of the header text, and what the tests hold the
HIP kernel (csrc/scvote_wide.hip.h) to."""
from __future__ import annotations

import numpy as np

from .resample import ERR_CLASS_BIT, ERR_DOMAIN_BIT, MAX_B, NUM_BINS, TIE_CLASSES, ResampleResult, dense_codes, truth_codes
from .synth import G, mix64

SEED_SALT = np.uint64(0x8EBC6AF09C88C6E3)
MAX_N = 4096                                    # SCV_WIDE_MAX_N; also the stride of a resample's key stream
_INDEX_MASK = np.uint64(MAX_N - 1)


def problem_streams(seed: int, pg) -> np.ndarray:
    """s_p = mix64((seed ^ 0x8EBC6AF09C88C6E3) + G * (pg + 1)) for global problem indices pg."""
    pg = np.asarray(pg, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64((np.uint64(seed) ^ SEED_SALT) + G * (pg + np.uint64(1)))


def sort_words(s, r, N: int) -> np.ndarray:
    """w_i = (mix64(s + G * (r * 4096 + i + 1)) & ~4095) | i for the resamples ``r`` of one problem stream ``s``: uint64 [len(r), N]."""
    r = np.asarray(r, dtype=np.uint64).reshape(-1, 1)
    i = np.arange(N, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        u = mix64(np.uint64(s) + G * (r * np.uint64(MAX_N) + i + np.uint64(1)))
    return (u & ~_INDEX_MASK) | i


def orderings(seed: int, pg: int, r, N: int) -> np.ndarray:
    """The orderings of problem ``pg`` for the resamples ``r``: int64 [len(r), N], every row a permutation of 0 .. N - 1."""
    w = sort_words(problem_streams(seed, pg), r, N)
    return np.argsort(w, axis=1, kind="stable").astype(np.int64)


def resample_wide(pool, truth, n_valid, r_begin: int, r_end: int, seed: int, tokens=None, p_offset: int = 0,
                  M: int | None = None, open_domain: bool = False) -> ResampleResult:
    """pool int32 [P, N] (1 <= N <= 4096), truth int32 [P], n_valid int32 [B] (budget b votes over the first clamp(n_valid[b], 0, N)
    samples of each ordering), resamples [r_begin, r_end).  ``M``: per_resample classes (None: not computed).  Votes outside 0..1023 count
    in bin 1023 and set error bit 0; a truth outside the bins never hits.
    ``open_domain`` (SCV_FLAG_OPEN_DOMAIN): every int32 is a value of its own -- a vote's bin is the rank of its value among the D <= N
    distinct values of its row, the truth hits when it equals a modal value, never error bit 0.  A hit with n_modes >= 1025 (D > 1024 only)
    has no column in tie_class_hits: it sets error bit 1 and is counted in neither table; its truth count and tokens are still added."""
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
    if open_domain:
        bins, uniq, _ = dense_codes(pool, True)
        tbin = truth_codes(uniq, truth, True)                            # the truth's bin, or -1
        nbins = [len(u) for u in uniq]
        err = 0
    else:
        v = pool.astype(np.int64)
        bad = (v < 0) | (v >= NUM_BINS)
        bins = np.where(bad, NUM_BINS - 1, v)
        tbin = np.where((truth >= 0) & (truth < NUM_BINS), truth, -1)
        nbins = [NUM_BINS] * P
        err = ERR_DOMAIN_BIT if bad.any() else 0
    if P * R == 0:
        return ResampleResult(P, R, tie, tsum, tcsum, per, err)
    tok_rows = None if tokens is None else np.asarray(tokens, dtype=np.int64)
    by_k = np.argsort(ks, kind="stable")
    kmax = int(ks.max())
    rs = np.arange(r_begin, r_end, dtype=np.int64)
    lane = np.arange(R)
    for p in range(P):
        order = orderings(seed, p_offset + p, rs, N)[:, :kmax]
        votes = bins[p][order]                                       # [R, kmax] in drawing order
        tok_cum = None if tok_rows is None else np.cumsum(tok_rows[p][order], axis=1)
        t, D = int(tbin[p]), nbins[p]
        cnt = np.zeros((R, D), dtype=np.int64)
        at = 0
        for b in by_k:
            k = int(ks[b])
            if k == 0:                                               # the empty prefix: no hit, nothing to add
                continue
            if k > at:
                cnt += np.bincount((lane[:, None] * D + votes[:, at:k]).reshape(-1), minlength=R * D).reshape(R, D)
                at = k
            maxc = cnt.max(axis=1)
            nmodes = (cnt == maxc[:, None]).sum(axis=1)
            tc = cnt[:, t] if t >= 0 else np.zeros(R, dtype=np.int64)
            hit = (tc == maxc) if t >= 0 else np.zeros(R, dtype=bool)
            if (nmodes[hit] >= TIE_CLASSES).any():                        # (open domain, D > 1024) no column for the class: counted nowhere
                err |= ERR_CLASS_BIT
                hit = hit & (nmodes < TIE_CLASSES)
            tie[b] += np.bincount(nmodes[hit], minlength=TIE_CLASSES)
            tcsum[b] += int(tc.sum())
            if tok_cum is not None:
                tsum[b] += int(tok_cum[:, k - 1].sum())
            if per is not None:
                m = nmodes[hit]
                if (m >= M).any():
                    err |= ERR_CLASS_BIT
                keep = m < M
                per[:, b, :] += np.bincount(lane[hit][keep] * M + m[keep], minlength=R * M).reshape(R, M)
    return ResampleResult(P, R, tie, tsum, tcsum, per, err)
