"""CPU mirror (numpy, uint64) of scv_iid_prefix_i32, spec in include/scvote.h: the majority vote over draws WITH replacement from each
problem's sample pool -- the plug-in (bootstrap) estimate of maj@k, defined past the size of the pool.  Vectorised over the (problem,
resample) lanes, one loop iteration per draw (the walk of resample.py, _mirror.running_mode_walk, with a draw where that one swaps); the same
role as resample.py -- the executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

import numpy as np

from ._mirror import ERR_DOMAIN_BIT, check_call, dense_codes, outputs, pool_shape, running_mode_walk, streams, truth_codes
from .resample import MAX_N, ResampleResult
from .synth import G, _MASK32, mix64

SEED_SALT = np.uint64(0xA0761D6478BD642F)
MAX_DRAWS = 65535                              # SCV_IID_MAX_DRAWS: a count fits 16 bits
R_STRIDE = 65536                               # counters of resample r: r * 65536 + 1 ... r * 65536 + 65535
ERR_DRAWS_BIT = 128                            # bit 7 of the device error word: a budget above MAX_DRAWS, nothing computed


def problem_streams(seed: int, pg) -> np.ndarray:
    """s_p = mix64((seed ^ 0xA0761D6478BD642F) + G * (pg + 1)) for global problem indices pg."""
    return streams(seed, SEED_SALT, pg)


def draw_index(s, r, i: int, N: int):
    """The pool index of draw i of resample r: mulhi32(hi32(mix64(s + G * (r * 65536 + i + 1))), N)."""
    with np.errstate(over="ignore"):
        u = mix64(np.asarray(s, dtype=np.uint64) + G * (np.asarray(r, dtype=np.uint64) * np.uint64(R_STRIDE) + np.uint64(i + 1)))
    return ((u >> np.uint64(32)) & _MASK32) * np.uint64(N) >> np.uint64(32)


def iid_prefix(pool, truth, n_draws, r_begin: int, r_end: int, seed: int, tokens=None, p_offset: int = 0, M: int = 0, open_domain: bool = False) -> ResampleResult:
    """pool int32 [P, N], truth int32 [P], n_draws int32 [B] (budget b votes over the first max(n_draws[b], 0) draws with replacement;
    not clamped to N, at most MAX_DRAWS), resamples [r_begin, r_end).  ``M``: per_resample classes (0: not computed).  A budget above
    MAX_DRAWS returns all-zero outputs with ERR_DRAWS_BIT in ``error_bits`` (what a DEVICE-mode call leaves; a HOST-mode call refuses)."""
    pool, P, N = pool_shape(pool)
    truth = np.asarray(truth, dtype=np.int64)
    nd = np.asarray(n_draws, dtype=np.int64).reshape(-1)
    _, _, R = check_call(P, N, nd.shape[0], r_begin, r_end, M, MAX_N, p_offset >= 0 and truth.shape == (P,), tail=f" p_offset={p_offset}", m_min=0)
    ks = np.maximum(nd, 0)
    tally, (tsum, tcsum), _ = outputs(P, nd.shape[0], R, M, 2)
    if P * R and ks.max() > MAX_DRAWS:
        tally.err = ERR_DRAWS_BIT
    elif P * R:
        codes, uniq, bad = dense_codes(pool, open_domain)
        tally.err = ERR_DOMAIN_BIT if bad else 0
        lp = np.repeat(np.arange(P), R)                                  # lanes problem-major
        lr = np.tile(np.arange(r_begin, r_end, dtype=np.int64), P)
        s, lru = problem_streams(seed, p_offset + lp), lr.astype(np.uint64)
        running_mode_walk(lambda i: draw_index(s, lru, i, N).astype(np.int64), codes, truth_codes(uniq, truth, open_domain)[lp],
                          None if tokens is None else np.asarray(tokens, dtype=np.int64), lp, lr - r_begin, ks, tally, tsum, tcsum)
    return ResampleResult(P, R, tally.tie, tsum, tcsum, tally.per, tally.err)
