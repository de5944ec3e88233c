"""CPU mirror (numpy) of scv_shortest_prefix_i32, spec in include/scvote.h: short-m@k, the majority vote over the m shortest of the first
k samples of a pool ordering.  The orderings are those of resample.py (token_budget.orderings: one definition of the shuffle); the kept
set comes from a stable sort of the prefix by (tokens, pool index), not from the kernel's bitmap over token ranks, so the two arrive at V by
different roads.  The executable statement of the header text, and what the tests hold the HIP kernel to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .resample import ERR_CLASS_BIT, ERR_DOMAIN_BIT, MAX_B, MAX_N, TIE_CLASSES, dense_codes, truth_codes
from .scoring import accuracy_from_tie_classes, exact_accuracy_from_tie_classes
from .token_budget import ERR_TOKEN_BIT, LANE_BLOCK, orderings


@dataclass
class ShortestResult:
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

    def _den(self):
        return self.P * self.R

    def _mean(self, total) -> np.float64:
        return np.float64(int(total)) / np.float64(self._den())

    def accuracy(self, b: int = 0) -> float:
        return accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def exact_accuracy(self, b: int = 0):
        return exact_accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def avg_voted_tokens(self, b: int = 0) -> np.float64:
        return self._mean(self.voted_token_sum[b])

    def avg_spent_tokens(self, b: int = 0) -> np.float64:
        return self._mean(self.spent_token_sum[b])

    def avg_latency(self, b: int = 0) -> np.float64:
        return self._mean(self.latency_sum[b])

    def resample_accuracy(self, b: int = 0) -> np.ndarray:
        """accuracy of every single ordering r: float64 [R]."""
        if self.per_resample is None:
            raise ValueError("per_resample was not requested")
        m = np.arange(1, self.per_resample.shape[2], dtype=np.float64)
        return (self.per_resample[:, b, 1:] / m).sum(axis=1) / self.P


def clamp_pairs(n_valid, m_keep, N: int):
    """(k_b, m_b) of the header: k_b = clamp(n_valid[b], 0, N), m_b = clamp(m_keep[b], 0, k_b); int64 [B] each."""
    k = np.clip(np.asarray(n_valid, dtype=np.int64).reshape(-1), 0, N)
    m = np.minimum(np.clip(np.asarray(m_keep, dtype=np.int64).reshape(-1), 0, None), k)
    return k, m


def shortest_prefix(pool, tokens, truth, n_valid, m_keep, r_begin: int = 0, r_end: int | None = None, seed: int = 0, p_offset: int = 0,
                    M: int | None = None, want_cells: bool = False, open_domain: bool = False) -> ShortestResult:
    """pool / tokens int32 [P, N], truth [P], n_valid / m_keep int32 [B].  ``r_end=None``: pool order (one draw, r_begin must be 0); otherwise
    the shuffled orderings r in [r_begin, r_end).  ``M``: per_resample classes (None: not computed).  ``want_cells``: pool order only."""
    pool = np.asarray(pool)
    if pool.ndim != 2:
        raise ValueError("pool must be [P, N]")
    P, N = pool.shape
    tok = np.asarray(tokens, dtype=np.int64)
    truth = np.asarray(truth, dtype=np.int64)
    if np.asarray(n_valid).reshape(-1).shape != np.asarray(m_keep).reshape(-1).shape:
        raise ValueError("n_valid and m_keep must both be [B]")
    ks, mk = clamp_pairs(n_valid, m_keep, N)
    B = ks.shape[0]
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
    vsum, ssum, lsum, tcsum = (np.zeros(B, dtype=np.int64) for _ in range(4))
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
        return ShortestResult(P, R, tie, vsum, ssum, lsum, tcsum, per, cells, cell_tokens, err)
    tcode = truth_codes(uniq, truth, open_domain)
    for l0 in range(0, L, LANE_BLOCK):
        l1 = min(L, l0 + LANE_BLOCK)
        lanes = np.arange(l0, l1)
        lp = lanes // R
        lr = lanes % R                                                  # relative to r_begin
        Lb = l1 - l0
        rows = np.arange(Lb)
        if shuffled:
            p_lo, p_hi = int(lp[0]), int(lp[-1]) + 1
            perm = orderings(p_hi - p_lo, N, r_begin, r_end, seed, p_offset + p_lo)[(lanes - p_lo * R)]
        else:
            perm = np.tile(np.arange(N, dtype=np.int64), (Lb, 1))
        key = tok[lp[:, None], perm] * N + perm                         # (tokens, pool index) as one integer: |tokens| < 2^31, index < N <= 256
        lt = tcode[lp]
        for b in range(B):
            k, m = int(ks[b]), int(mk[b])
            if m == 0:
                continue                                                # the empty cell: no hit, 0 in every sum, an all-zero record
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
            tie[b] += np.bincount(nm[hit], minlength=TIE_CLASSES)[:TIE_CLASSES]
            tcsum[b] += int(tc.sum())
            vsum[b] += int(voted.sum())
            ssum[b] += int(spent.sum())
            lsum[b] += int(t_m.sum())
            if per is not None:
                c = nm[hit]
                if (c >= M).any():
                    err |= ERR_CLASS_BIT
                keep = c < M
                per[:, b, :] += np.bincount(lr[hit][keep] * M + c[keep], minlength=R * M).reshape(R, M)
            if cells is not None:
                mc = modal.argmax(axis=1)                               # the smallest modal code
                cells["max_count"][lp, b] = mx
                cells["truth_count"][lp, b] = tc
                cells["n_modes"][lp, b] = nm
                cells["min_mode"][lp, b] = [int(c) if open_domain else int(uniq[p][c]) for p, c in zip(lp.tolist(), mc.tolist())]
                cells["hit"][lp, b] = hit
                cell_tokens[lp, b] = spent
        if cells is not None:
            for b in range(B):
                if mk[b] == 0:
                    cells["min_mode"][lp, b] = -1
    return ShortestResult(P, R, tie, vsum, ssum, lsum, tcsum, per, cells, cell_tokens, err)
