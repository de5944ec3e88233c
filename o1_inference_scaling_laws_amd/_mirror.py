"""What the numpy mirrors of the ordering votes share (resample, iid, wide, wide_budget, token_budget, weighted, adaptive, shortest), each piece
once: the constants of the device error word and of the tie table, the methods of the result classes, the stream seeding, the call checks, the
zeroed outputs, the tally of hits, the lane blocks, the cell records, the dense codes and the running-mode walk.  A mirror keeps what makes it
that vote and reads top to bottom as its header text; nothing here knows which vote calls it.  The index functions (swap_index, draw_index)
and ``orderings`` are arguments, looked up by the caller in its own module at call time: the tests replace them there."""
from __future__ import annotations

import numpy as np

from .scoring import accuracy_from_tie_classes, exact_accuracy_from_tie_classes
from .synth import G, mix64

NUM_BINS, TIE_CLASSES = 1024, 1025
MAX_B = 32
ERR_DOMAIN_BIT, ERR_CLASS_BIT = 1, 2           # bits of the device error word (include/scvote.h)


class VoteResult:
    """The methods every result dataclass of the ordering votes has; no fields.  Every denominator is P * R (cells per budget)."""

    def _den(self):
        return self.P * self.R

    def _mean(self, total) -> np.float64:
        return np.float64(int(total)) / np.float64(self._den())

    def accuracy(self, b: int = 0) -> float:
        return accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def exact_accuracy(self, b: int = 0):
        return exact_accuracy_from_tie_classes(self.tie_class_hits[b], self._den())

    def resample_accuracy(self, b: int = 0) -> np.ndarray:
        """accuracy of every single ordering r (its spread is the noise of a one-ordering curve): float64 [R]."""
        if self.per_resample is None:
            raise ValueError("per_resample was not requested")
        m = np.arange(1, self.per_resample.shape[2], dtype=np.float64)
        return (self.per_resample[:, b, 1:] / m).sum(axis=1) / self.P


def streams(seed: int, salt, pg) -> np.ndarray:
    """s_p = mix64((seed ^ salt) + G * (pg + 1)) for global problem indices pg."""
    pg = np.asarray(pg, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64((np.uint64(seed) ^ salt) + G * (pg + np.uint64(1)))


def pool_shape(pool):
    """(pool as an array, P, N); anything but [P, N] is refused."""
    pool = np.asarray(pool)
    if pool.ndim != 2:
        raise ValueError("pool must be [P, N]")
    return pool, pool.shape[0], pool.shape[1]


def check_call(P: int, N: int, B: int, r_begin: int, r_end, M, max_n: int, shapes_ok: bool, has_order: bool = False, want_cells: bool = False,
               refusal: str | None = None, tail: str = "", m_min: int = 1):
    """The refusals every mirror shares, in the order of the header: the pool-order rule (``has_order``: ``r_end=None`` is the pool order, one
    draw), the caller's own ``refusal`` (a text, or None), the ranges of N, B and r with ``shapes_ok`` (the caller's test of its other arrays),
    cells outside the pool order, M below ``m_min``.  Returns (shuffled, r_end, R)."""
    shuffled = not has_order or r_end is not None
    if not shuffled:
        if r_begin != 0:
            raise ValueError("pool order is one draw: r_begin must be 0")
        r_end = 1
    if refusal is not None:
        raise ValueError(refusal)
    if not (1 <= N <= max_n and 1 <= B <= MAX_B and 0 <= r_begin <= r_end < 2 ** 31 and shapes_ok):
        raise ValueError(f"bad shape P={P} N={N} B={B} r=[{r_begin},{r_end}){tail}")
    if want_cells and shuffled:
        raise ValueError("cells are written in pool order only")
    if M is not None and M < m_min:
        raise ValueError(f"M must be >= {m_min}")
    return shuffled, r_end, r_end - r_begin


class Tally:
    """tie_class_hits [B, 1025], per_resample [R, B, M] (None when ``M`` is None or 0) and the error bits of one call."""

    def __init__(self, B: int, R: int, M, err: int = 0):
        self.R, self.M, self.err = R, M, err
        self.tie = np.zeros((B, TIE_CLASSES), dtype=np.int64)
        self.per = np.zeros((R, B, M), dtype=np.int64) if M else None

    def add(self, b: int, n_modes, hit, r_rel) -> None:
        """The lanes of ``hit`` into the tables of budget b, each by its class n_modes and -- per_resample -- its resample r_rel (relative to
        r_begin).  A class without a column in per_resample (n_modes >= M) raises ERR_CLASS_BIT and is left out of that table."""
        m = n_modes[hit]
        self.tie[b] += np.bincount(m, minlength=TIE_CLASSES)[:TIE_CLASSES]
        if self.per is not None:
            R, M = self.R, self.M
            if (m >= M).any():
                self.err |= ERR_CLASS_BIT
            keep = m < M
            self.per[:, b, :] += np.bincount(r_rel[hit][keep] * M + m[keep], minlength=R * M).reshape(R, M)


def outputs(P: int, B: int, R: int, M, n_sums: int, want_cells: bool = False, min_mode: int = 0, err: int = 0):
    """The zeroed outputs of a call: (Tally, ``n_sums`` int64 [B] sums, CELL_DTYPE [P, B] records or None); an unwritten record has
    ``min_mode`` in its min_mode field."""
    cells = None
    if want_cells:
        from .engine import CELL_DTYPE
        cells = np.zeros((P, B), dtype=CELL_DTYPE)
        cells["min_mode"] = min_mode
    return Tally(B, R, M, err), [np.zeros(B, dtype=np.int64) for _ in range(n_sums)], cells


def lane_blocks(P: int, R: int, N: int, block: int, orderings, shuffled: bool, r_begin: int, r_end: int, seed: int, p_offset: int):
    """The (problem, resample) lanes, problem-major, in blocks of ``block``: yields (lp, lr, perm) -- the lanes' problems, their resamples
    relative to r_begin, and their orderings int64 [lanes, N]: those of ``orderings`` (the caller's, token_budget.orderings) or the pool order."""
    for l0 in range(0, P * R, block):
        lanes = np.arange(l0, min(P * R, l0 + block))
        lp, lr = lanes // R, lanes % R
        if shuffled:
            # the orderings of this block's problems (a block starts and ends inside rows: take the whole rows and cut)
            p_lo, p_hi = int(lp[0]), int(lp[-1]) + 1
            perm = orderings(p_hi - p_lo, N, r_begin, r_end, seed, p_offset + p_lo)[lanes - p_lo * R]
        else:
            perm = np.tile(np.arange(N, dtype=np.int64), (len(lanes), 1))
        yield lp, lr, perm


def write_cells(cells, lp, b: int, mx, tc, nm, mc, hit, live, uniq=None) -> None:
    """The records of budget b of the problems ``lp`` (pool order: one lane per problem).  ``mc`` is the smallest modal code: written through
    ``uniq`` (the rows' sorted distinct values) or, without it, as it is; a cell that is not ``live`` (no vote counted) has no mode: -1."""
    cells["max_count"][lp, b] = mx
    cells["truth_count"][lp, b] = tc
    cells["n_modes"][lp, b] = nm
    cells["min_mode"][lp, b] = [(int(c) if uniq is None else int(uniq[p][c])) if ok else -1
                                for p, c, ok in zip(np.asarray(lp).tolist(), np.asarray(mc).tolist(), np.asarray(live).tolist())]
    cells["hit"][lp, b] = hit


def dense_codes(pool: np.ndarray, open_domain: bool = False):
    """Votes outside 0..1023 -> bin 1023 (and a flag); then each row re-encoded to value-ordered dense codes.
    Returns (codes int64 [P, N], sorted distinct values per row (list), domain flag).
    ``open_domain`` (SCV_FLAG_OPEN_DOMAIN): every int32 is a value of its own, in signed order -- no clamp, never a domain flag."""
    v = np.asarray(pool, dtype=np.int64)
    if open_domain:
        v = np.asarray(pool).astype(np.int32).astype(np.int64)
        bad = np.zeros(v.shape, dtype=bool)
    else:
        bad = (v < 0) | (v >= NUM_BINS)
    v = np.where(bad, NUM_BINS - 1, v)
    codes = np.empty_like(v)
    uniq = []
    for p in range(v.shape[0]):
        u, inv = np.unique(v[p], return_inverse=True)
        codes[p] = inv.reshape(-1)
        uniq.append(u)
    return codes, uniq, bool(bad.any())


def truth_codes(uniq, truth, open_domain: bool = False) -> np.ndarray:
    """The truth's code in its row (``uniq``: the rows' sorted distinct values, from dense_codes), or -1: absent, or -- without
    ``open_domain`` -- outside the bins (such a truth never hits)."""
    tcode = np.full(len(uniq), -1, dtype=np.int64)
    for p, u in enumerate(uniq):
        t = int(truth[p])
        if open_domain or 0 <= t < NUM_BINS:
            k = np.searchsorted(u, t)
            if k < len(u) and u[k] == t:
                tcode[p] = k
    return tcode


def wide_bins(pool, truth, open_domain: bool):
    """The bins of the wide pair: (bins int64 [P, N], the truth's bin or -1 [P], bins per row (list), the domain error bit or 0).  Closed domain:
    a vote is its own bin, outside 0..1023 bin 1023 and the bit; open domain: the rank of its value among the distinct values of its row."""
    if open_domain:
        bins, uniq, _ = dense_codes(pool, True)
        return bins, truth_codes(uniq, truth, True), [len(u) for u in uniq], 0
    v = pool.astype(np.int64)
    bad = (v < 0) | (v >= NUM_BINS)
    tbin = np.where((truth >= 0) & (truth < NUM_BINS), truth, -1)
    return np.where(bad, NUM_BINS - 1, v), tbin, [NUM_BINS] * pool.shape[0], ERR_DOMAIN_BIT if bad.any() else 0


def running_mode_walk(pick, codes, ltc, tok_rows, lp, r_rel, ks, tally: Tally, tsum, tcsum) -> None:
    """One lane per (problem, resample), one step per sample: ``pick(i)`` gives every lane's pool index of sample i, the lane's count table, its
    mode count and number of modes follow, and every budget is tallied when the walk reaches its length ``ks[b]`` (budgets in sorted order).
    ``ltc``: the lanes' truth codes; ``tok_rows``: tokens [P, N] or None."""
    L, B = lp.shape[0], ks.shape[0]
    cnt = np.zeros((L, codes.shape[1]), dtype=np.int32)
    maxc = np.zeros(L, dtype=np.int32)
    nmodes = np.zeros(L, dtype=np.int32)
    tc = np.zeros(L, dtype=np.int64)
    tok = np.zeros(L, dtype=np.int64)
    lanes = np.arange(L)
    order = np.argsort(ks, kind="stable")
    q = 0
    while q < B and ks[order[q]] == 0:                               # empty cells: no hit, nothing to add
        q += 1
    for i in range(int(ks.max())):
        x = pick(i)
        code = codes[lp, x]
        c = cnt[lanes, code] + 1
        cnt[lanes, code] = c
        gt, eq = c > maxc, c == maxc
        nmodes = np.where(gt, 1, np.where(eq, nmodes + 1, nmodes))
        maxc = np.where(gt, c, maxc)
        tc += code == ltc
        if tok_rows is not None:
            tok += tok_rows[lp, x]
        while q < B and ks[order[q]] == i + 1:
            b = int(order[q])
            tally.add(b, nmodes, (ltc >= 0) & (tc == maxc), r_rel)
            tcsum[b] += int(tc.sum())
            tsum[b] += int(tok.sum())
            q += 1
