"""CPU mirror (numpy, uint64) of scv_iid_prefix_i32, spec in include/scvote.h: the majority vote over draws WITH replacement from each
problem's sample pool -- the plug-in (bootstrap) estimate of maj@k, defined past the size of the pool.  Vectorised over the (problem,
resample) lanes, one loop iteration per draw; the same role as resample.py -- the executable statement of the header text, and what the
tests hold the HIP kernel to."""
from __future__ import annotations

import numpy as np

from .resample import ERR_CLASS_BIT, ERR_DOMAIN_BIT, MAX_B, MAX_N, NUM_BINS, TIE_CLASSES, ResampleResult, dense_codes, truth_codes
from .synth import G, _MASK32, mix64

SEED_SALT = np.uint64(0xA0761D6478BD642F)
MAX_DRAWS = 65535                              # SCV_IID_MAX_DRAWS: a count fits 16 bits
R_STRIDE = 65536                               # counters of resample r: r * 65536 + 1 ... r * 65536 + 65535
ERR_DRAWS_BIT = 128                            # bit 7 of the device error word: a budget above MAX_DRAWS, nothing computed


def problem_streams(seed: int, pg) -> np.ndarray:
    """s_p = mix64((seed ^ 0xA0761D6478BD642F) + G * (pg + 1)) for global problem indices pg."""
    pg = np.asarray(pg, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64((np.uint64(seed) ^ SEED_SALT) + G * (pg + np.uint64(1)))


def draw_index(s, r, i: int, N: int):
    """The pool index of draw i of resample r: mulhi32(hi32(mix64(s + G * (r * 65536 + i + 1))), N)."""
    with np.errstate(over="ignore"):
        u = mix64(np.asarray(s, dtype=np.uint64) + G * (np.asarray(r, dtype=np.uint64) * np.uint64(R_STRIDE) + np.uint64(i + 1)))
    return ((u >> np.uint64(32)) & _MASK32) * np.uint64(N) >> np.uint64(32)


def iid_prefix(pool, truth, n_draws, r_begin: int, r_end: int, seed: int, tokens=None, p_offset: int = 0, M: int = 0, open_domain: bool = False) -> ResampleResult:
    """pool int32 [P, N], truth int32 [P], n_draws int32 [B] (budget b votes over the first max(n_draws[b], 0) draws with replacement;
    not clamped to N, at most MAX_DRAWS), resamples [r_begin, r_end).  ``M``: per_resample classes (0: not computed).  A budget above
    MAX_DRAWS returns all-zero outputs with ERR_DRAWS_BIT in ``error_bits`` (what a DEVICE-mode call leaves; a HOST-mode call refuses)."""
    pool = np.asarray(pool)
    if pool.ndim != 2:
        raise ValueError("pool must be [P, N]")
    P, N = pool.shape
    truth = np.asarray(truth, dtype=np.int64)
    nd = np.asarray(n_draws, dtype=np.int64).reshape(-1)
    B = nd.shape[0]
    if not (1 <= N <= MAX_N and 1 <= B <= MAX_B and 0 <= r_begin <= r_end < 2 ** 31 and p_offset >= 0) or truth.shape != (P,):
        raise ValueError(f"bad shape P={P} N={N} B={B} r=[{r_begin},{r_end}) p_offset={p_offset}")
    if M < 0:
        raise ValueError("M must be >= 0")
    R = r_end - r_begin
    ks = np.maximum(nd, 0)
    tie = np.zeros((B, TIE_CLASSES), dtype=np.int64)
    tsum = np.zeros(B, dtype=np.int64)
    tcsum = np.zeros(B, dtype=np.int64)
    per = np.zeros((R, B, M), dtype=np.int64) if M else None
    L = P * R
    if L == 0:
        return ResampleResult(P, R, tie, tsum, tcsum, per, 0)
    if ks.max() > MAX_DRAWS:
        return ResampleResult(P, R, tie, tsum, tcsum, per, ERR_DRAWS_BIT)
    codes, uniq, bad = dense_codes(pool, open_domain)
    err = ERR_DOMAIN_BIT if bad else 0
    tcode = truth_codes(uniq, truth, open_domain)
    lp = np.repeat(np.arange(P), R)                                  # lanes problem-major
    lr = np.tile(np.arange(r_begin, r_end, dtype=np.int64), P)
    s = problem_streams(seed, p_offset + lp)
    lru = lr.astype(np.uint64)
    ltc = tcode[lp]
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
    while q < B and ks[order[q]] == 0:                               # empty cells: no hit, nothing to add
        q += 1
    for i in range(kmax):
        x = draw_index(s, lru, i, N).astype(np.int64)
        code = codes[lp, x]
        c = cnt[lanes, code] + 1
        cnt[lanes, code] = c
        gt, eq = c > maxc, c == maxc
        nmodes = np.where(gt, 1, np.where(eq, nmodes + 1, nmodes))
        maxc = np.where(gt, c, maxc)
        tc += code == ltc
        if tok_rows is not None:
            tok += tok_rows[lp, x]
        while q < B and ks[order[q]] == i + 1:
            b = int(order[q])
            hit = (ltc >= 0) & (tc == maxc)
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
