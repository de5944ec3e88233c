"""CPU mirror (numpy) of scv_token_budget_prefix_i32, spec in include/scvote.h: the majority vote over the longest prefix of a pool
ordering that fits a budget of tokens.  The orderings are those of resample.py (problem_streams / swap_index: one definition of the
shuffle); the prefix lengths come from a cumulative sum and a binary search per ordering, not from the kernel's running test, so the two
arrive at n_b by different roads.  The executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .resample import ERR_CLASS_BIT, ERR_DOMAIN_BIT, MAX_B, MAX_N, NUM_BINS, TIE_CLASSES, dense_codes, truth_codes, problem_streams, swap_index
from .scoring import accuracy_from_tie_classes, avg_tokens_used, exact_accuracy_from_tie_classes

ORDER_POOL, ORDER_SHUFFLED = 0, 1
ERR_TOKEN_BIT = 16                              # bit 4 of the device error word: a negative token count
LANE_BLOCK = 4096                               # lanes per block of the mirror (bounds its [lanes, N + 1] state tables)


@dataclass
class TokenBudgetResult:
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

    def _den(self):
        return self.P * self.R

    def accuracy(self, b: int = 0) -> float:
        return accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def exact_accuracy(self, b: int = 0):
        return exact_accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def avg_tokens_used(self, b: int = 0) -> np.float64:
        return avg_tokens_used(self.token_sum[b], self._den())

    def avg_votes(self, b: int = 0) -> np.float64:
        return np.float64(int(self.vote_count_sum[b])) / np.float64(self._den())

    def resample_accuracy(self, b: int = 0) -> np.ndarray:
        """accuracy of every single ordering r: float64 [R]."""
        if self.per_resample is None:
            raise ValueError("per_resample was not requested")
        m = np.arange(1, self.per_resample.shape[2], dtype=np.float64)
        return (self.per_resample[:, b, 1:] / m).sum(axis=1) / self.P


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
    pool = np.asarray(pool)
    if pool.ndim != 2:
        raise ValueError("pool must be [P, N]")
    P, N = pool.shape
    tok = np.asarray(tokens, dtype=np.int64)
    truth = np.asarray(truth, dtype=np.int64)
    T = np.asarray(token_budgets, dtype=np.int64).reshape(-1)
    B = T.shape[0]
    shuffled = r_end is not None
    if not shuffled:
        if r_begin != 0:
            raise ValueError("pool order is one draw: r_begin must be 0")
        r_end = 1
    if not (1 <= N <= MAX_N and 1 <= B <= MAX_B and 0 <= r_begin <= r_end < 2 ** 31) or truth.shape != (P,) or tok.shape != pool.shape:
        raise ValueError(f"bad shape P={P} N={N} B={B} r=[{r_begin},{r_end})")
    if want_cells and shuffled:
        raise ValueError("cells are written in pool order only")
    if M is not None and M < 1:
        raise ValueError("M must be >= 1")
    R = r_end - r_begin
    tie = np.zeros((B, TIE_CLASSES), dtype=np.int64)
    tsum = np.zeros(B, dtype=np.int64)
    vsum = np.zeros(B, dtype=np.int64)
    tcsum = np.zeros(B, dtype=np.int64)
    per = np.zeros((R, B, M), dtype=np.int64) if M is not None else None
    cells = cell_tokens = None
    if want_cells:
        from .engine import CELL_DTYPE
        cells = np.zeros((P, B), dtype=CELL_DTYPE)
        cell_tokens = np.zeros((P, B), dtype=np.int64)
    codes, uniq, bad = dense_codes(pool, open_domain)
    err = (ERR_DOMAIN_BIT if bad else 0) | (ERR_TOKEN_BIT if (tok < 0).any() else 0)
    L = P * R
    if L == 0:
        return TokenBudgetResult(P, R, tie, tsum, vsum, tcsum, per, cells, cell_tokens, err)
    tcode = truth_codes(uniq, truth, open_domain)
    for l0 in range(0, L, LANE_BLOCK):
        l1 = min(L, l0 + LANE_BLOCK)
        lanes = np.arange(l0, l1)
        lp = lanes // R
        lr = lanes % R                                                  # relative to r_begin
        Lb = l1 - l0
        if shuffled:
            # the orderings of this block's problems (a block starts and ends inside rows: take the whole rows and cut)
            p_lo, p_hi = int(lp[0]), int(lp[-1]) + 1
            perm = orderings(p_hi - p_lo, N, r_begin, r_end, seed, p_offset + p_lo)[(lanes - p_lo * R)]
        else:
            perm = np.tile(np.arange(N, dtype=np.int64), (Lb, 1))
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
            tie[b] += np.bincount(nm[hit], minlength=TIE_CLASSES)[:TIE_CLASSES]
            tcsum[b] += int(tc.sum())
            tsum[b] += int(S[rows, nb].sum())
            vsum[b] += int(nb.sum())
            if per is not None:
                m = nm[hit]
                if (m >= M).any():
                    err |= ERR_CLASS_BIT
                keep = m < M
                per[:, b, :] += np.bincount(lr[hit][keep] * M + m[keep], minlength=R * M).reshape(R, M)
            if cells is not None:
                mc = minc[rows, nb]
                cells["max_count"][lp, b] = mx
                cells["truth_count"][lp, b] = tc
                cells["n_modes"][lp, b] = nm
                cells["min_mode"][lp, b] = [(int(k) if open_domain else int(uniq[p][k])) if k >= 0 else -1 for p, k in zip(lp.tolist(), mc.tolist())]
                cells["hit"][lp, b] = hit
                cell_tokens[lp, b] = S[rows, nb]
    return TokenBudgetResult(P, R, tie, tsum, vsum, tcsum, per, cells, cell_tokens, err)
