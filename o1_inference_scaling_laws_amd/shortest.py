"""CPU mirror (numpy) of scv_shortest_prefix_i32, spec in include/scvote.h: short-m@k, the majority vote over the m shortest of the first
k samples of a pool ordering.  The orderings are those of token_budget.orderings (the one definition of the shuffle, over
resample.swap_index), block by block through _mirror.lane_blocks; the kept set comes from a stable sort of the prefix by (tokens, pool index),
not from the kernel's bitmap over token ranks, so the two arrive at V by different roads.  The executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._mirror import ERR_DOMAIN_BIT, VoteResult, check_call, dense_codes, lane_blocks, outputs, pool_shape, truth_codes, write_cells
from .resample import MAX_N
from .token_budget import ERR_TOKEN_BIT, LANE_BLOCK, orderings


@dataclass
class ShortestResult(VoteResult):
    """Integer outputs of one short-m@k call + the floats derived from them.  Every denominator is P * R (cells per budget; R = 1 in pool
    order): accuracy(b) is short-m_b@k_b averaged over problems (and orderings); the three token means are per cell."""
    P: int
    R: int
    tie_class_hits: np.ndarray          # int64 [B, 1025]
    voted_token_sum: np.ndarray         # int64 [B]: tokens of the kept samples
    spent_token_sum: np.ndarray         # int64 [B]: ... plus (k - m) * t_(m): what the k parallel samples cost
    latency_sum: np.ndarray             # int64 [B]: t_(m), the length of the m-th shortest chain
    truth_count_sum: np.ndarray         # int64 [B]
    per_resample: np.ndarray | None     # int64 [R, B, M]
    cells: np.ndarray | None = None     # CELL_DTYPE [P, B] (pool order)
    cell_tokens: np.ndarray | None = None   # int64 [P, B] (pool order): the cell's spent tokens
    error_bits: int = 0                 # bit 0: a vote outside 0..1023; bit 1: a hit with n_modes >= M; bit 4: a negative token

    def avg_voted_tokens(self, b: int = 0) -> np.float64:
        return self._mean(self.voted_token_sum[b])

    def avg_spent_tokens(self, b: int = 0) -> np.float64:
        return self._mean(self.spent_token_sum[b])

    def avg_latency(self, b: int = 0) -> np.float64:
        return self._mean(self.latency_sum[b])


def clamp_pairs(n_valid, m_keep, N: int):
    """(k_b, m_b) of the header: k_b = clamp(n_valid[b], 0, N), m_b = clamp(m_keep[b], 0, k_b); int64 [B] each."""
    k = np.clip(np.asarray(n_valid, dtype=np.int64).reshape(-1), 0, N)
    m = np.minimum(np.clip(np.asarray(m_keep, dtype=np.int64).reshape(-1), 0, None), k)
    return k, m


def shortest_prefix(pool, tokens, truth, n_valid, m_keep, r_begin: int = 0, r_end: int | None = None, seed: int = 0, p_offset: int = 0,
                    M: int | None = None, want_cells: bool = False, open_domain: bool = False) -> ShortestResult:
    """pool / tokens int32 [P, N], truth [P], n_valid / m_keep int32 [B].  ``r_end=None``: pool order (one draw, r_begin must be 0); otherwise
    the shuffled orderings r in [r_begin, r_end).  ``M``: per_resample classes (None: not computed).  ``want_cells``: pool order only."""
    pool, P, N = pool_shape(pool)
    tok = np.asarray(tokens, dtype=np.int64)
    truth = np.asarray(truth, dtype=np.int64)
    if np.asarray(n_valid).reshape(-1).shape != np.asarray(m_keep).reshape(-1).shape:
        raise ValueError("n_valid and m_keep must both be [B]")
    ks, mk = clamp_pairs(n_valid, m_keep, N)
    B = ks.shape[0]
    shuffled, r_end, R = check_call(P, N, B, r_begin, r_end, M, MAX_N, truth.shape == (P,) and tok.shape == pool.shape, True, want_cells)
    codes, uniq, bad = dense_codes(pool, open_domain)
    err = (ERR_DOMAIN_BIT if bad else 0) | (ERR_TOKEN_BIT if (tok < 0).any() else 0)
    tally, (vsum, ssum, lsum, tcsum), cells = outputs(P, B, R, M, 4, want_cells, err=err)
    cell_tokens = np.zeros((P, B), dtype=np.int64) if want_cells else None
    tcode = truth_codes(uniq, truth, open_domain)
    for lp, lr, perm in lane_blocks(P, R, N, LANE_BLOCK, orderings, shuffled, r_begin, r_end, seed, p_offset):
        Lb = lp.shape[0]
        rows = np.arange(Lb)
        key = tok[lp[:, None], perm] * N + perm                         # (tokens, pool index) as one integer: |tokens| < 2^31, index < N <= 256
        lt = tcode[lp]
        for b in range(B):
            k, m = int(ks[b]), int(mk[b])
            if m == 0:                                                  # the empty cell: no hit, 0 in every sum, an all-zero record without a mode
                if cells is not None:
                    cells["min_mode"][lp, b] = -1
                continue
            front = np.argsort(key[:, :k], axis=1, kind="stable")[:, :m]
            V = perm[rows[:, None], front]                              # [Lb, m] pool indices, shortest first
            vc = codes[lp[:, None], V]
            vt = tok[lp[:, None], V]
            cnt = np.zeros((Lb, N), dtype=np.int64)
            np.add.at(cnt, (rows[:, None], vc), 1)
            mx = cnt.max(axis=1)
            modal = cnt == mx[:, None]
            nm = modal.sum(axis=1)
            tc = np.where(lt >= 0, cnt[rows, np.maximum(lt, 0)], 0)
            hit = (lt >= 0) & (tc == mx)
            voted = vt.sum(axis=1)
            t_m = vt[:, -1]
            spent = voted + (k - m) * t_m
            tally.add(b, nm, hit, lr)
            tcsum[b] += int(tc.sum())
            vsum[b] += int(voted.sum())
            ssum[b] += int(spent.sum())
            lsum[b] += int(t_m.sum())
            if cells is not None:                                       # (modal.argmax: the smallest modal code; m >= 1: every cell has a mode)
                write_cells(cells, lp, b, mx, tc, nm, modal.argmax(axis=1), hit, mx > 0, None if open_domain else uniq)
                cell_tokens[lp, b] = spent
    return ShortestResult(P, R, tally.tie, vsum, ssum, lsum, tcsum, tally.per, cells, cell_tokens, tally.err)
