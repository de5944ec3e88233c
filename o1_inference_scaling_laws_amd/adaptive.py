"""CPU mirror (numpy) of scv_adaptive_prefix_i32, spec in include/scvote.h: the majority vote that samples until a stopping rule says it is
settled.  The orderings are those of token_budget.orderings (the one definition of the shuffle, over resample.swap_index), block by block
through _mirror.lane_blocks.  For every prefix length the mirror tabulates c1 and c2 from the two largest counts (np.partition over the count vector -- the header's "second value in descending
order of count", not the kernel's running runner-up) and finds each rule's stopping point as the first true entry of a condition table, not
from a running mask of open rules: mirror and kernel arrive at n by different roads.  The rule builders (never, margin_rule, beta_rule) are
host-only and exact integers.  The executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from math import comb

import numpy as np

from ._mirror import ERR_DOMAIN_BIT, VoteResult, check_call, dense_codes, lane_blocks, outputs, pool_shape, truth_codes, write_cells
from .resample import MAX_N
from .scoring import avg_tokens_used
from .token_budget import orderings

STOP_DECIDED = 0x1
ERR_RULE_FLAG_BIT = 64                          # bit 6 of the device error word: a rule flag with an unknown bit
LANE_BLOCK = 2048                               # lanes per block of the mirror (bounds its [lanes, N + 1] state tables)


def never(N: int) -> np.ndarray:
    """need[c2] = N + 1 for every c2: condition (a) never holds; with flag 0 the rule is the fixed vote over the cap."""
    return np.full(N + 1, N + 1, dtype=np.int32)


def margin_rule(N: int, m: int) -> np.ndarray:
    """need[c2] = c2 + m: stop at a lead of m votes over the runner-up (the call clamps to 0 .. N + 1: above N means never)."""
    return (np.arange(N + 1, dtype=np.int64) + int(m)).astype(np.int32)


def beta_confidence(c1: int, c2: int) -> Fraction:
    """P(p1 > p2) under Beta(c1 + 1, c2 + 1): sum_{j=0..c1} C(c1 + c2 + 1, j) / 2^(c1 + c2 + 1), exact."""
    n = c1 + c2 + 1
    return Fraction(sum(comb(n, j) for j in range(c1 + 1)), 1 << n)


def beta_rule(N: int, conf) -> np.ndarray:
    """The Adaptive-Consistency criterion: need[c2] = the smallest c1 in c2 + 1 .. N with beta_confidence(c1, c2) >= conf, N + 1 when there
    is none.  The confidence rises with c1 and falls with c2 (it is P(Binomial(c1 + c2 + 1, 1/2) >= c2 + 1)), so need is non-decreasing in
    c2 and the search for c2 starts where the one for c2 - 1 ended."""
    conf = Fraction(conf)
    need = np.full(N + 1, N + 1, dtype=np.int32)
    c1 = 1
    for c2 in range(N + 1):
        c1 = max(c1, c2 + 1)
        while c1 <= N and beta_confidence(c1, c2) < conf:
            c1 += 1
        if c1 > N:
            break
        need[c2] = c1
    return need


@dataclass
class AdaptiveResult(VoteResult):
    """Integer outputs of one adaptive call + the floats derived from them.  Every denominator is P * R (cells per rule; R = 1 in pool
    order): accuracy(b) is the vote under rule b averaged over problems (and orderings), avg_votes(b) / avg_tokens_used(b) what it spent."""
    P: int
    R: int
    tie_class_hits: np.ndarray          # int64 [B, 1025]
    token_sum: np.ndarray | None        # int64 [B] (None without tokens)
    vote_count_sum: np.ndarray          # int64 [B]: samples drawn
    truth_count_sum: np.ndarray         # int64 [B]
    stop_hist: np.ndarray               # int64 [B, N + 1]: cells that stopped after n samples
    per_resample: np.ndarray | None     # int64 [R, B, M]
    cells: np.ndarray | None = None     # CELL_DTYPE [P, B] (pool order)
    cell_tokens: np.ndarray | None = None   # int64 [P, B] (pool order, with tokens)
    cell_votes: np.ndarray | None = None    # int32 [P, B] (pool order)
    error_bits: int = 0                 # bit 0: a vote outside 0..1023; bit 1: a hit with n_modes >= M; bit 6: an unknown rule flag

    def avg_tokens_used(self, b: int = 0) -> np.float64:
        if self.token_sum is None:
            raise ValueError("tokens were not given")
        return avg_tokens_used(self.token_sum[b], self._den())

    def avg_votes(self, b: int = 0) -> np.float64:
        return self._mean(self.vote_count_sum[b])

    def stop_distribution(self, b: int = 0) -> np.ndarray:
        """share of the cells of rule b that stopped after n = 0 .. N samples: float64 [N + 1]."""
        return self.stop_hist[b].astype(np.float64) / np.float64(self._den())


def check_rules(cap, need, rule_flags, N: int):
    """(cap int32 [B], need int32 [B, N + 1], flags int32 [B]) as contiguous arrays; a single need row is repeated for every cap."""
    cap = np.ascontiguousarray(cap, dtype=np.int32).reshape(-1)
    B = cap.shape[0]
    need = np.ascontiguousarray(need, dtype=np.int32)
    if need.ndim == 1:
        need = np.ascontiguousarray(np.tile(need, (B, 1)))
    flags = np.zeros(B, dtype=np.int32) if rule_flags is None else np.ascontiguousarray(rule_flags, dtype=np.int32).reshape(-1)
    if need.shape != (B, N + 1) or flags.shape != (B,):
        raise ValueError(f"cap must be [B], need [B, N + 1] and rule_flags [B] (B={B}, N={N}; got need {need.shape}, flags {flags.shape})")
    return cap, need, flags


def adaptive_prefix(pool, truth, cap, need, rule_flags=None, tokens=None, r_begin: int = 0, r_end: int | None = None, seed: int = 0,
                    p_offset: int = 0, M: int | None = None, want_cells: bool = False, open_domain: bool = False) -> AdaptiveResult:
    """pool int32 [P, N], truth [P], cap int32 [B], need int32 [B, N + 1], rule_flags int32 [B] or None, tokens [P, N] or None.
    ``r_end=None``: pool order (one draw, r_begin must be 0); otherwise the shuffled orderings r in [r_begin, r_end).  ``M``: per_resample
    classes (None: not computed).  ``want_cells``: pool order only."""
    pool, P, N = pool_shape(pool)
    truth = np.asarray(truth, dtype=np.int64)
    cap, need, flags = check_rules(cap, need, rule_flags, N)
    B = cap.shape[0]
    tok = None if tokens is None else np.asarray(tokens, dtype=np.int64)
    shuffled, r_end, R = check_call(P, N, B, r_begin, r_end, M, MAX_N, truth.shape == (P,) and (tok is None or tok.shape == pool.shape), True, want_cells)
    nmax = np.clip(cap.astype(np.int64), 0, N)
    need = np.clip(need.astype(np.int64), 0, N + 1)
    codes, uniq, bad = dense_codes(pool, open_domain)
    err = (ERR_DOMAIN_BIT if bad else 0) | (ERR_RULE_FLAG_BIT if (flags & ~STOP_DECIDED).any() else 0)
    tally, (tsum, vsum, tcsum), cells = outputs(P, B, R, M, 3, want_cells, err=err)
    tsum = tsum if tok is not None else None
    hist = np.zeros((B, N + 1), dtype=np.int64)
    cell_tokens = np.zeros((P, B), dtype=np.int64) if want_cells and tok is not None else None
    cell_votes = np.zeros((P, B), dtype=np.int32) if want_cells else None
    tcode = truth_codes(uniq, truth, open_domain)
    ns = np.arange(N + 1, dtype=np.int64)
    for lp, lr, perm in lane_blocks(P, R, N, LANE_BLOCK, orderings, shuffled, r_begin, r_end, seed, p_offset):
        Lb = lp.shape[0]
        x_codes = codes[lp[:, None], perm]
        S = np.zeros((Lb, N + 1), dtype=np.int64)
        if tok is not None:
            S[:, 1:] = np.cumsum(tok[lp[:, None], perm], axis=1)
        # the statistics of every prefix length 0 .. N: c1 / c2 from the two largest counts, the number of modes, the smallest modal code
        c1 = np.zeros((Lb, N + 1), dtype=np.int64)
        c2 = np.zeros((Lb, N + 1), dtype=np.int64)
        nmod = np.zeros((Lb, N + 1), dtype=np.int64)
        tcs = np.zeros((Lb, N + 1), dtype=np.int64)
        minc = np.full((Lb, N + 1), -1, dtype=np.int64)
        cnt = np.zeros((Lb, N), dtype=np.int64)
        rows = np.arange(Lb)
        for i in range(N):
            c = x_codes[:, i]
            cnt[rows, c] += 1
            if N >= 2:
                top = -np.partition(-cnt, 1, axis=1)[:, :2]
                c1[:, i + 1], c2[:, i + 1] = top[:, 0], top[:, 1]
            else:
                c1[:, i + 1] = cnt[:, 0]
            modal = cnt == c1[:, i + 1, None]
            nmod[:, i + 1] = modal.sum(axis=1)
            minc[:, i + 1] = modal.argmax(axis=1)
            tcs[:, i + 1] = tcs[:, i] + (c == tcode[lp])
        for b in range(B):
            k = int(nmax[b])
            cond = c1 >= need[b][c2]                                    # (a)
            if flags[b] & STOP_DECIDED:
                cond |= (c1 - c2) > (k - ns)[None, :]                   # (b)
            cond[:, 0] = False
            cond[:, k] = True                                           # (c); k == 0: the empty cell
            cond[:, k + 1:] = False
            nb = cond.argmax(axis=1)
            mx, nm, tc = c1[rows, nb], nmod[rows, nb], tcs[rows, nb]
            hit = (tc > 0) & (tc == mx)
            tally.add(b, nm, hit, lr)
            tcsum[b] += int(tc.sum())
            vsum[b] += int(nb.sum())
            hist[b] += np.bincount(nb, minlength=N + 1)
            if tsum is not None:
                tsum[b] += int(S[rows, nb].sum())
            if cells is not None:
                write_cells(cells, lp, b, mx, tc, nm, minc[rows, nb], hit, nb > 0, None if open_domain else uniq)
                cell_votes[lp, b] = nb
                if cell_tokens is not None:
                    cell_tokens[lp, b] = S[rows, nb]
    return AdaptiveResult(P, R, tally.tie, tsum, vsum, tcsum, hist, tally.per, cells, cell_tokens, cell_votes, tally.err)
