"""CPU mirror (numpy) of scv_token_budget_prefix_i32, spec in include/scvote.h: the majority vote over the longest prefix of a pool
ordering that fits a budget of tokens.  The orderings are those of resample.py (``orderings`` below walks resample's problem_streams /
swap_index: the one definition of the shuffle, which _mirror.lane_blocks cuts into blocks for this mirror and the three after it; what all
mirrors share is in _mirror.py); the prefix lengths come from a cumulative sum and a binary search per ordering, not from the kernel's running test, so the two
arrive at n_b by different roads.  The executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._mirror import ERR_DOMAIN_BIT, VoteResult, check_call, dense_codes, lane_blocks, outputs, pool_shape, truth_codes, write_cells
from .resample import MAX_N, problem_streams, swap_index
from .scoring import avg_tokens_used

ORDER_POOL, ORDER_SHUFFLED = 0, 1
ERR_TOKEN_BIT = 16                              # bit 4 of the device error word: a negative token count
LANE_BLOCK = 4096                               # lanes per block of the mirror (bounds its [lanes, N + 1] state tables)


@dataclass
class TokenBudgetResult(VoteResult):
    """Integer outputs of one token-budget call + the floats derived from them.  Every denominator is P * R (cells per budget; R = 1 in
    pool order): accuracy(b) is the maj vote at T_b averaged over problems (and orderings), avg_tokens_used(b) the tokens it spent."""
    P: int
    R: int
    tie_class_hits: np.ndarray          # int64 [B, 1025]
    token_sum: np.ndarray               # int64 [B]: tokens spent
    vote_count_sum: np.ndarray          # int64 [B]: sum of n_b
    truth_count_sum: np.ndarray         # int64 [B]
    per_resample: np.ndarray | None     # int64 [R, B, M]
    cells: np.ndarray | None = None     # CELL_DTYPE [P, B] (pool order)
    cell_tokens: np.ndarray | None = None   # int64 [P, B] (pool order)
    error_bits: int = 0                 # bit 0: a vote outside 0..1023; bit 1: a hit with n_modes >= M; bit 4: a negative token

    def avg_tokens_used(self, b: int = 0) -> np.float64:
        return avg_tokens_used(self.token_sum[b], self._den())

    def avg_votes(self, b: int = 0) -> np.float64:
        return self._mean(self.vote_count_sum[b])


def orderings(P: int, N: int, r_begin: int, r_end: int, seed: int, p_offset: int = 0) -> np.ndarray:
    """The partial Fisher-Yates permutations of scv_resample_prefix_i32 for every (problem, r), lanes problem-major: int64 [P * R, N]."""
    R = r_end - r_begin
    lp = np.repeat(np.arange(P), R)
    lr = np.tile(np.arange(r_begin, r_end, dtype=np.uint64), P)
    s = problem_streams(seed, p_offset + lp)
    perm = np.tile(np.arange(N, dtype=np.int64), (P * R, 1))
    lanes = np.arange(P * R)
    for i in range(N - 1):
        j = swap_index(s, lr, i, N).astype(np.int64)
        x = perm[lanes, j]
        perm[lanes, j] = perm[:, i]
        perm[:, i] = x
    return perm


def token_budget_prefix(pool, tokens, truth, token_budgets, r_begin: int = 0, r_end: int | None = None, seed: int = 0,
                        p_offset: int = 0, M: int | None = None, want_cells: bool = False, open_domain: bool = False) -> TokenBudgetResult:
    """pool / tokens int32 [P, N], truth [P], token_budgets int64 [B].  ``r_end=None``: pool order (one draw, r_begin must be 0); otherwise
    the shuffled orderings r in [r_begin, r_end).  ``M``: per_resample classes (None: not computed).  ``want_cells``: pool order only."""
    pool, P, N = pool_shape(pool)
    tok = np.asarray(tokens, dtype=np.int64)
    truth = np.asarray(truth, dtype=np.int64)
    T = np.asarray(token_budgets, dtype=np.int64).reshape(-1)
    B = T.shape[0]
    shuffled, r_end, R = check_call(P, N, B, r_begin, r_end, M, MAX_N, truth.shape == (P,) and tok.shape == pool.shape, True, want_cells)
    codes, uniq, bad = dense_codes(pool, open_domain)
    err = (ERR_DOMAIN_BIT if bad else 0) | (ERR_TOKEN_BIT if (tok < 0).any() else 0)
    tally, (tsum, vsum, tcsum), cells = outputs(P, B, R, M, 3, want_cells, err=err)
    cell_tokens = np.zeros((P, B), dtype=np.int64) if want_cells else None
    tcode = truth_codes(uniq, truth, open_domain)
    for lp, lr, perm in lane_blocks(P, R, N, LANE_BLOCK, orderings, shuffled, r_begin, r_end, seed, p_offset):
        Lb = lp.shape[0]
        x_codes = codes[lp[:, None], perm]
        S = np.zeros((Lb, N + 1), dtype=np.int64)
        S[:, 1:] = np.cumsum(tok[lp[:, None], perm], axis=1)
        n = np.empty((Lb, B), dtype=np.int64)
        for k in range(Lb):
            n[k] = np.maximum(np.searchsorted(S[k], T, side="right") - 1, 0)
        # the mode statistics of every prefix length 0 .. N
        maxc = np.zeros((Lb, N + 1), dtype=np.int64)
        nmod = np.zeros((Lb, N + 1), dtype=np.int64)
        tcs = np.zeros((Lb, N + 1), dtype=np.int64)
        minc = np.full((Lb, N + 1), -1, dtype=np.int64)
        cnt = np.zeros((Lb, N), dtype=np.int64)
        rows = np.arange(Lb)
        for i in range(N):
            c = x_codes[:, i]
            v = cnt[rows, c] + 1
            cnt[rows, c] = v
            m0, k0, mc0 = maxc[:, i], nmod[:, i], minc[:, i]
            gt, eq = v > m0, v == m0
            maxc[:, i + 1] = np.where(gt, v, m0)
            nmod[:, i + 1] = np.where(gt, 1, np.where(eq, k0 + 1, k0))
            minc[:, i + 1] = np.where(gt, c, np.where(eq, np.minimum(mc0, c), mc0))
            tcs[:, i + 1] = tcs[:, i] + (c == tcode[lp])
        for b in range(B):
            nb = n[:, b]
            mx, nm, tc = maxc[rows, nb], nmod[rows, nb], tcs[rows, nb]
            hit = (tc > 0) & (tc == mx)
            tally.add(b, nm, hit, lr)
            tcsum[b] += int(tc.sum())
            tsum[b] += int(S[rows, nb].sum())
            vsum[b] += int(nb.sum())
            if cells is not None:
                mc = minc[rows, nb]
                write_cells(cells, lp, b, mx, tc, nm, mc, hit, mc >= 0, None if open_domain else uniq)
                cell_tokens[lp, b] = S[rows, nb]
    return TokenBudgetResult(P, R, tally.tie, tsum, vsum, tcsum, tally.per, cells, cell_tokens, tally.err)
