"""CPU mirror (numpy, uint64) of scv_resample_prefix_i32, spec in include/scvote.h: the expected majority vote over random
orderings of each problem's sample pool.  Vectorised over the (problem, resample) lanes, one loop iteration per Fisher-Yates
step; the same role as synth.py -- the executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._mirror import ERR_CLASS_BIT, ERR_DOMAIN_BIT, MAX_B, NUM_BINS, TIE_CLASSES, dense_codes, truth_codes  # noqa: F401 (tests and tools read them here)
from ._mirror import VoteResult, check_call, outputs, pool_shape, running_mode_walk, streams
from .scoring import avg_tokens_used
from .synth import G, _MASK32, mix64

SEED_SALT = np.uint64(0xD6E8FEB86659FD93)
MAX_N = 256


def problem_streams(seed: int, pg) -> np.ndarray:
    """s_p = mix64((seed ^ 0xD6E8FEB86659FD93) + G * (pg + 1)) for global problem indices pg."""
    return streams(seed, SEED_SALT, pg)


def swap_index(s, r, i: int, N: int):
    """j of Fisher-Yates step i of resample r: i + mulhi32(hi32(mix64(s + G * (r * N + i + 1))), N - i)."""
    with np.errstate(over="ignore"):
        u = mix64(np.asarray(s, dtype=np.uint64) + G * (np.asarray(r, dtype=np.uint64) * np.uint64(N) + np.uint64(i + 1)))
    return np.uint64(i) + (((u >> np.uint64(32)) & _MASK32) * np.uint64(N - i) >> np.uint64(32))


@dataclass
class ResampleResult(VoteResult):
    """Integer outputs of one resampled-majority call + the floats derived from them.  Every denominator is
    P * R (cells per budget): accuracy(b) is the expected maj@k_b over orderings, averaged over problems."""
    P: int
    R: int
    tie_class_hits: np.ndarray          # int64 [B, 1025]
    token_sum: np.ndarray               # int64 [B]
    truth_count_sum: np.ndarray         # int64 [B]
    per_resample: np.ndarray | None     # int64 [R, B, M]: class counts of each ordering, summed over problems
    error_bits: int = 0                 # bit 0: a vote outside 0..1023; bit 1: a hit with n_modes >= M

    def avg_tokens_used(self, b: int = 0) -> np.float64:
        return avg_tokens_used(self.token_sum[b], self._den())


def resample_prefix(pool, truth, n_valid, r_begin: int, r_end: int, seed: int, tokens=None, p_offset: int = 0,
                    M: int | None = None, open_domain: bool = False) -> ResampleResult:
    """pool int32 [P, N], truth int32 [P], n_valid int32 [B] (budget b votes over the first clamp(n_valid[b], 0, N) of a
    random ordering), resamples [r_begin, r_end).  ``M``: per_resample classes (None: not computed)."""
    pool, P, N = pool_shape(pool)
    truth = np.asarray(truth, dtype=np.int64)
    nv = np.asarray(n_valid, dtype=np.int64).reshape(-1)
    _, _, R = check_call(P, N, nv.shape[0], r_begin, r_end, M, MAX_N, truth.shape == (P,))
    ks = np.clip(nv, 0, N)
    codes, uniq, bad = dense_codes(pool, open_domain)
    tally, (tsum, tcsum), _ = outputs(P, nv.shape[0], R, M, 2, err=ERR_DOMAIN_BIT if bad else 0)
    L = P * R
    if L:
        lp = np.repeat(np.arange(P), R)                                  # lanes problem-major
        lr = np.tile(np.arange(r_begin, r_end, dtype=np.int64), P)
        s, lru = problem_streams(seed, p_offset + lp), lr.astype(np.uint64)
        perm = np.tile(np.arange(N, dtype=np.int16), (L, 1))
        lanes = np.arange(L)

        def pick(i):                                                     # Fisher-Yates step i: sample i of every lane's ordering
            j = swap_index(s, lru, i, N).astype(np.int64)
            x = perm[lanes, j].astype(np.int64)
            perm[lanes, j] = perm[:, i]
            perm[:, i] = x
            return x

        running_mode_walk(pick, codes, truth_codes(uniq, truth, open_domain)[lp], None if tokens is None else np.asarray(tokens, dtype=np.int64),
                          lp, lr - r_begin, ks, tally, tsum, tcsum)
    return ResampleResult(P, R, tally.tie, tsum, tcsum, tally.per, tally.err)
