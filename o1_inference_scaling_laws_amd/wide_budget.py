"""CPU mirror (numpy) of scv_token_budget_wide_i32, spec in include/scvote.h: the majority vote over the longest prefix of an ordering of a
pool of up to 4096 samples that fits a budget of tokens.  The orderings are those of wide.py (``wide.orderings``: the one definition of the sort
words; the bins of the pair are _mirror.wide_bins), the result type that of token_budget.py; the prefix lengths come from ``cumsum`` plus ``searchsorted`` per ordering, not from the
kernel's packed words and binary search.  The executable statement of the header text, and what the tests hold the HIP kernel
(csrc/scvote_wide_budget.hip.h) to."""
from __future__ import annotations

import numpy as np

from ._mirror import ERR_CLASS_BIT, TIE_CLASSES, check_call, outputs, pool_shape, wide_bins, write_cells
from .token_budget import ERR_TOKEN_BIT, ORDER_POOL, ORDER_SHUFFLED, TokenBudgetResult
from .wide import MAX_N, orderings

__all__ = ["token_budget_wide", "prefix_lengths", "ORDER_POOL", "ORDER_SHUFFLED"]


def prefix_lengths(tok_in_order: np.ndarray, budgets: np.ndarray) -> np.ndarray:
    """n_b = max { n <= N : sum_{i<n} tok[i] <= T_b } for every row of ``tok_in_order`` (int64 [L, N], no negative entry) and every budget
    (int64 [B]): int64 [L, B].  The sums do not decrease, so n_b is the number of running sums that are <= T_b."""
    S = np.cumsum(tok_in_order, axis=1, dtype=np.int64)
    return np.stack([np.searchsorted(S[k], budgets, side="right") for k in range(S.shape[0])]).astype(np.int64).reshape(S.shape[0], -1)


def token_budget_wide(pool, tokens, truth, token_budgets, r_begin: int = 0, r_end: int | None = None, seed: int = 0, p_offset: int = 0,
                      M: int | None = None, want_cells: bool = False, open_domain: bool = False) -> TokenBudgetResult:
    """pool / tokens int32 [P, N] (1 <= N <= 4096), truth [P], token_budgets int64 [B].  ``r_end=None``: pool order (one draw, r_begin must be
    0); otherwise the orderings r in [r_begin, r_end) of ``wide.resample_wide``.  ``M``: per_resample classes (None: not computed).
    ``want_cells``: pool order only.  Votes outside 0..1023 count in bin 1023 and set error bit 0; a truth outside the bins never hits.
    ``open_domain`` (SCV_FLAG_OPEN_DOMAIN): every int32 is a value of its own -- a vote's bin is the rank of its value among the D <= N
    distinct values of its row, min_mode of a cell is that rank, never error bit 0.  A hit with n_modes >= 1025 (D > 1024 only) has no column
    in tie_class_hits: it sets error bit 1 and is counted in neither table; its sums are still added.  A negative token count sets error bit
    4 and is added as 0."""
    pool, P, N = pool_shape(pool)
    tok = np.asarray(tokens, dtype=np.int64)
    truth = np.asarray(truth, dtype=np.int64)
    T = np.asarray(token_budgets, dtype=np.int64).reshape(-1)
    B = T.shape[0]
    shuffled, r_end, R = check_call(P, N, B, r_begin, r_end, M, MAX_N, truth.shape == (P,) and tok.shape == pool.shape, True, want_cells)
    bins, tbin, nbins, err = wide_bins(pool, truth, open_domain)
    tally, (tsum, vsum, tcsum), cells = outputs(P, B, R, M, 3, want_cells, min_mode=-1, err=err | (ERR_TOKEN_BIT if (tok < 0).any() else 0))
    cell_tokens = np.zeros((P, B), dtype=np.int64) if want_cells else None
    tok = np.maximum(tok, 0)                                             # (the kernel adds a negative count as 0 after raising the bit)
    rs = np.arange(r_begin, r_end, dtype=np.int64)
    lane = np.arange(R)
    for p in range(P if R else 0):
        order = orderings(seed, p_offset + p, rs, N) if shuffled else np.arange(N, dtype=np.int64).reshape(1, N)
        tok_o = tok[p][order]                                            # [R, N] in drawing order
        S = np.zeros((R, N + 1), dtype=np.int64)
        S[:, 1:] = np.cumsum(tok_o, axis=1)
        n = prefix_lengths(tok_o, T)                                     # [R, B]
        votes = bins[p][order]
        t, D = int(tbin[p]), nbins[p]
        # every distinct prefix length of the problem once, ascending: the counts of each ordering grow from one length to the next
        cnt = np.zeros((R, D), dtype=np.int64)
        at = np.zeros(R, dtype=np.int64)
        for b in np.argsort(n.max(axis=0), kind="stable"):               # (any order of the budgets gives the same sums; this one keeps `at` small)
            nb = n[:, b]
            for r in range(R):                                           # orderings end at different lengths: one row at a time
                k = int(nb[r])
                if k > at[r]:
                    cnt[r] += np.bincount(votes[r, at[r]:k], minlength=D)
                    at[r] = k
                elif k < at[r]:                                          # a budget that is shorter in this ordering than one walked before
                    cnt[r] = np.bincount(votes[r, :k], minlength=D)
                    at[r] = k
            live = nb > 0                                                # the empty prefix: no hit, nothing to add
            maxc = cnt.max(axis=1)
            nmodes = (cnt == maxc[:, None]).sum(axis=1)
            tc = cnt[:, t] if t >= 0 else np.zeros(R, dtype=np.int64)
            hit = live & (tc == maxc) if t >= 0 else np.zeros(R, dtype=bool)
            counted = hit
            if (nmodes[hit] >= TIE_CLASSES).any():                       # (open domain, D > 1024) no column for the class: counted nowhere
                tally.err |= ERR_CLASS_BIT
                counted = hit & (nmodes < TIE_CLASSES)
            tally.add(b, nmodes, counted, lane)
            tcsum[b] += int(tc[live].sum())
            tsum[b] += int(S[lane, nb].sum())
            vsum[b] += int(nb.sum())
            if cells is not None and live[0]:                            # pool order: R = 1; an empty cell keeps its all-zero record, min_mode -1
                # the smallest modal bin: the value, or -- open domain -- its code
                write_cells(cells, [p], b, maxc, tc, nmodes, [int(np.argmax(cnt[0] == maxc[0]))], hit, live)
                cell_tokens[p, b] = S[0, nb[0]]
    return TokenBudgetResult(P, R, tally.tie, tsum, vsum, tcsum, tally.per, cells, cell_tokens, tally.err)
