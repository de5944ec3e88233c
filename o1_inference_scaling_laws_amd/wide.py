"""CPU mirror (numpy, uint64) of scv_resample_wide_i32, spec in include/scvote.h: the expected majority vote over random orderings
of pools of up to 4096 samples.  An ordering is defined by sort keys, not by a Fisher-Yates walk: one np.argsort over the uint64 words of
every resample of a problem.  The same role as resample.py -- the executable statement of the header text, and what the tests hold the
HIP kernel (csrc/scvote_wide.hip.h) to."""
from __future__ import annotations

import numpy as np

from ._mirror import ERR_CLASS_BIT, TIE_CLASSES, check_call, outputs, pool_shape, streams, wide_bins
from .resample import ResampleResult
from .synth import G, mix64

SEED_SALT = np.uint64(0x8EBC6AF09C88C6E3)
MAX_N = 4096                                    # SCV_WIDE_MAX_N; also the stride of a resample's key stream
_INDEX_MASK = np.uint64(MAX_N - 1)


def problem_streams(seed: int, pg) -> np.ndarray:
    """s_p = mix64((seed ^ 0x8EBC6AF09C88C6E3) + G * (pg + 1)) for global problem indices pg."""
    return streams(seed, SEED_SALT, pg)


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
    pool, P, N = pool_shape(pool)
    truth = np.asarray(truth, dtype=np.int64)
    nv = np.asarray(n_valid, dtype=np.int64).reshape(-1)
    _, _, R = check_call(P, N, nv.shape[0], r_begin, r_end, M, MAX_N, truth.shape == (P,))
    ks = np.clip(nv, 0, N)
    bins, tbin, nbins, err = wide_bins(pool, truth, open_domain)
    tally, (tsum, tcsum), _ = outputs(P, nv.shape[0], R, M, 2, err=err)
    tok_rows = None if tokens is None else np.asarray(tokens, dtype=np.int64)
    by_k = np.argsort(ks, kind="stable")
    kmax = int(ks.max())
    rs = np.arange(r_begin, r_end, dtype=np.int64)
    lane = np.arange(R)
    for p in range(P if R else 0):
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
                tally.err |= ERR_CLASS_BIT
                hit = hit & (nmodes < TIE_CLASSES)
            tally.add(b, nmodes, hit, lane)
            tcsum[b] += int(tc.sum())
            if tok_cum is not None:
                tsum[b] += int(tok_cum[:, k - 1].sum())
    return ResampleResult(P, R, tally.tie, tsum, tcsum, tally.per, tally.err)
