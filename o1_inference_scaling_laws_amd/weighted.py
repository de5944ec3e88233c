"""CPU mirror (numpy) of scv_weighted_prefix_i32, spec in include/scvote.h: the weighted majority vote (rule 0: a value's weight is the sum
of its samples' weights) and best-of-N (rule 1: the maximum) over the prefixes of a pool ordering.  The orderings are those of
token_budget.orderings (the one definition of the shuffle, over resample.swap_index), block by block through _mirror.lane_blocks.  Every
prefix's W(v) is built from scratch with np.add.at / np.maximum.at over the prefix's samples, not by the kernel's running rule, so the two
arrive at the modes by different roads.  The executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._mirror import ERR_DOMAIN_BIT, VoteResult, check_call, dense_codes, lane_blocks, outputs, pool_shape, truth_codes, write_cells
from .resample import MAX_N
from .scoring import avg_tokens_used
from .token_budget import orderings

RULE_WEIGHT_SUM, RULE_BEST_OF = 0, 1
WEIGHT_MAX = 2 ** 24 - 1
ERR_WEIGHT_BIT = 32                             # bit 5 of the device error word: a weight outside 0 .. WEIGHT_MAX
LANE_BLOCK = 4096                               # lanes per block of the mirror (bounds its [lanes, N] tables)


@dataclass
class WeightedResult(VoteResult):
    """Integer outputs of one weighted-vote call + the floats derived from them.  Every denominator is P * R (cells per budget; R = 1 in
    pool order): accuracy(b) is the weighted vote (or best-of-N) over k_b samples averaged over problems (and orderings)."""
    P: int
    R: int
    tie_class_hits: np.ndarray          # int64 [B, 1025]
    token_sum: np.ndarray | None        # int64 [B]: tokens of the samples in the prefixes (None without tokens)
    per_resample: np.ndarray | None     # int64 [R, B, M]
    cells: np.ndarray | None = None     # CELL_DTYPE [P, B] (pool order): max_count = the top weight, truth_count = the truth's weight
    cell_tokens: np.ndarray | None = None   # int64 [P, B] (pool order, with tokens)
    error_bits: int = 0                 # bit 0: a vote outside 0..1023; bit 1: a hit with n_modes >= M; bit 5: a weight out of range

    def avg_tokens_used(self, b: int = 0) -> np.float64:
        return avg_tokens_used(0 if self.token_sum is None else self.token_sum[b], self._den())


def quantize_weights(scores, lo=None, hi=None) -> np.ndarray:
    """Float scores -> int32 weights in 0 .. WEIGHT_MAX: w = floor((clip(s, lo, hi) - lo) / (hi - lo) * WEIGHT_MAX + 0.5) in float64 (round
    half up), so lo -> 0, hi -> WEIGHT_MAX and s1 <= s2 gives w1 <= w2.  ``lo`` / ``hi`` default to the smallest / largest score; when they
    coincide every weight is WEIGHT_MAX (all samples vote alike).  NaN is refused.  Scores closer than (hi - lo) / 2^24 may share a weight:
    a tie the exact scores would not have had."""
    s = np.asarray(scores, dtype=np.float64)
    if np.isnan(s).any():
        raise ValueError("scores contain NaN")
    lo = (float(s.min()) if s.size else 0.0) if lo is None else float(lo)
    hi = (float(s.max()) if s.size else 0.0) if hi is None else float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
        raise ValueError(f"bad range lo={lo} hi={hi}")
    if hi == lo:
        return np.full(s.shape, WEIGHT_MAX, dtype=np.int32)
    u = (np.clip(s, lo, hi) - lo) / (hi - lo)
    return np.floor(u * WEIGHT_MAX + 0.5).astype(np.int32)


def weighted_prefix(pool, weights, truth, n_valid, rule: int = RULE_WEIGHT_SUM, r_begin: int = 0, r_end: int | None = None, seed: int = 0,
                    p_offset: int = 0, M: int | None = None, tokens=None, want_cells: bool = False, open_domain: bool = False) -> WeightedResult:
    """pool / weights int32 [P, N], truth [P], n_valid int32 [B].  ``r_end=None``: pool order (one draw, r_begin must be 0); otherwise the
    shuffled orderings r in [r_begin, r_end).  ``M``: per_resample classes (None: not computed).  ``want_cells``: pool order only."""
    pool, P, N = pool_shape(pool)
    if weights is None:
        raise ValueError("weights are required")
    wts = np.asarray(weights, dtype=np.int64)
    truth = np.asarray(truth, dtype=np.int64)
    nv = np.asarray(n_valid, dtype=np.int64).reshape(-1)
    B = nv.shape[0]
    tok = None if tokens is None else np.asarray(tokens, dtype=np.int64)
    shapes_ok = p_offset >= 0 and truth.shape == (P,) and wts.shape == pool.shape and (tok is None or tok.shape == pool.shape)
    shuffled, r_end, R = check_call(P, N, B, r_begin, r_end, M, MAX_N, shapes_ok, True, want_cells,
                                    refusal=None if rule in (RULE_WEIGHT_SUM, RULE_BEST_OF) else f"bad rule {rule}")
    ks = np.clip(nv, 0, N)
    codes, uniq, bad = dense_codes(pool, open_domain)
    wbad = (wts < 0) | (wts > WEIGHT_MAX)
    err = (ERR_DOMAIN_BIT if bad else 0) | (ERR_WEIGHT_BIT if wbad.any() else 0)
    tally, (tsum,), cells = outputs(P, B, R, M, 1, want_cells, min_mode=-1, err=err)
    tsum = tsum if tok is not None else None
    cell_tokens = np.zeros((P, B), dtype=np.int64) if want_cells and tok is not None else None
    wts = wts & WEIGHT_MAX                                              # what the kernel counts after it raised the bit (results are invalid)
    tcode = truth_codes(uniq, truth, open_domain)
    for lp, lr, perm in lane_blocks(P, R, N, LANE_BLOCK, orderings, shuffled, r_begin, r_end, seed, p_offset):
        Lb = lp.shape[0]
        x_codes = codes[lp[:, None], perm]
        x_w = wts[lp[:, None], perm]
        x_tok = None if tok is None else tok[lp[:, None], perm]
        rows = np.arange(Lb)
        tc_lane = tcode[lp]
        for b in range(B):
            k = int(ks[b])
            W = np.zeros((Lb, N), dtype=np.int64)                        # by row code, from scratch for this prefix
            if k:
                idx = (np.repeat(rows, k), x_codes[:, :k].reshape(-1))
                (np.add if rule == RULE_WEIGHT_SUM else np.maximum).at(W, idx, x_w[:, :k].reshape(-1))
            top = W.max(axis=1)
            is_mode = (W == top[:, None]) & (top[:, None] > 0)
            nm = is_mode.sum(axis=1)
            tw = np.where(tc_lane >= 0, W[rows, np.maximum(tc_lane, 0)], 0)
            hit = (tw > 0) & (tw == top)
            tally.add(b, nm, hit, lr)
            spent = None if x_tok is None else x_tok[:, :k].sum(axis=1)
            if tsum is not None:
                tsum[b] += int(spent.sum())
            if cells is not None:
                mc = is_mode.argmax(axis=1)                              # the smallest modal code: codes are value-ordered
                write_cells(cells, lp, b, top, tw, nm, mc, hit, top > 0, None if open_domain else uniq)
                if cell_tokens is not None:
                    cell_tokens[lp, b] = spent
    return WeightedResult(P, R, tally.tie, tsum, tally.per, cells, cell_tokens, tally.err)
