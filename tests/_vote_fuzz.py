"""Seeded draws for the ordering, draw and exact votes (scv_resample_prefix_i32, scv_token_budget_prefix_i32, scv_weighted_prefix_i32,
scv_adaptive_prefix_i32, scv_iid_prefix_i32, scv_expected_majority_i32): ``draw(entry, seed)`` returns one complete, VALID call -- host
arrays, scalars, mode flags -- that depends on (entry, seed) alone; ``mirror_outputs`` runs the entry's numpy mirror on it; ``lanes_that_fit``
restates the five *_lds_words formulas of csrc/scvote_dispatch.h.  No GPU, no torch: tests/test_vote_fuzz_cpu.py checks what the draws reach,
tests/test_gpu_fuzz_votes.py holds the kernels to them.

The five lane bodies share one kernel and state their LDS layout twice (device carving, host formula); the launch shape (256 / 128 / 64 lanes,
np_max = min(P, (lanes - 1) / R + 2)) moves with N, B, R, P and the order.  So the draws couple what a one-axis-at-a-time list cannot: the
edges of N, B and R are weighted, one draw in seven comes from the "tight" regime (N >= 252 with B >= 31 or with R <= 3 and P >= 300:
the layouts where 256 or 128 lanes stop fitting), and P is drawn by the lanes it makes (fewer than 64, a ragged few chunks, many chunks).

Work bound: P * R * (largest budget, or N) <= WORK[entry] // work_div."""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from o1_inference_scaling_laws_amd import adaptive, iid, resample, synth, token_budget, weighted

LANE_ENTRIES = ("resample", "token_budget", "weighted", "adaptive", "iid")
ENTRIES = LANE_ENTRIES + ("expected",)
HAS_ORDER = ("token_budget", "weighted", "adaptive")
STREAM = {e: 7_100_000 + 1000 * i for i, e in enumerate(ENTRIES)}       # one default_rng stream per entry: default_rng((STREAM[entry], seed))
DEFAULT_VOTE_SEEDS = 120                                                 # seeds per lane entry that tests/test_gpu_fuzz_votes.py runs by default and
                                                                         # tests/test_vote_fuzz_cpu.py proves its reach conditions on
WORK = {"resample": 1_500_000, "token_budget": 1_500_000, "weighted": 1_500_000, "adaptive": 300_000, "iid": 1_500_000, "expected": 0}

N_EDGES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 253, 255, 256)
N_EDGE_P = np.array([3.0 if n in (1, 256) else 1.0 for n in N_EDGES]) / (len(N_EDGES) + 4)      # the two ends of the range: three shares each
B_EDGES = (1, 2, 31, 32)
R_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)
TRUTH_ODD = (1023, -3, 2000)
WEIGHT_MAX = 2 ** 24 - 1
LDS_MAX_BYTES = 160 * 1024                                               # gfx950: one workgroup may declare all of it

SUMMED = ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "stop_hist", "per_resample")      # DEVICE mode: +=
WRITTEN = ("cells", "cell_tokens", "cell_votes")                                                                  # overwritten in both modes
CELL_FIELDS = ("max_count", "truth_count", "n_modes", "min_mode", "hit")


# ---- the layouts, restated from csrc/scvote_dispatch.h ---------------------------------------------------------------------------------------

def lds_words(entry: str, N: int, B: int, lanes: int, np_max: int, shuffled: bool, R: int) -> int:
    N4, waves = (N + 3) // 4, lanes // 64
    rows = 2 * np_max + np_max * N4
    if entry == "resample":
        return 4 * B + B * (N + 1) + 64 + 64 * waves + rows + 2 * lanes * N4
    if entry == "token_budget":
        return 64 + 6 * B + 32 + B * (N + 1) + 64 * waves + rows + (2 if shuffled else 1) * lanes * N4
    if entry == "adaptive":
        return 6 * B + 32 + 2 + 2 * B * (N + 1) + (B * (N + 1) + 1) // 2 + 64 * waves + rows + (2 if shuffled else 1) * lanes * N4
    if entry == "iid":
        return 4 * B + B * (N + 1) + 64 + 64 * waves + rows + lanes * ((N + 1) // 2)
    if entry == "weighted":
        wlds = shuffled and R >= 64
        return 2 * B + B * (N + 1) + 64 + 64 * waves + 2 * np_max + np_max * (N if wlds else N4) + lanes * N + (lanes * N4 if shuffled else 0)
    raise KeyError(entry)


def lanes_that_fit(entry: str, N: int, B: int, R: int, P: int, shuffled: bool):
    """The workgroup sizes of launch_lane_body whose layout fits the LDS of one workgroup (the occupancy query then picks among them)."""
    return tuple(lanes for lanes in (256, 128, 64)
                 if 4 * lds_words(entry, N, B, lanes, min(P, (lanes - 1) // R + 2), shuffled, R) <= LDS_MAX_BYTES)


def fit_class(case) -> str:
    fit = lanes_that_fit(case.entry, case.N, case.B, case.R, case.P, case.shuffled)
    return "256" if 256 in fit else ("128" if 128 in fit else "64")


# ---- the pieces of a draw ---------------------------------------------------------------------------------------------------------------

def _pick(rng, edges, p_edge, lo, hi):
    return int(rng.choice(edges)) if rng.random() < p_edge else int(rng.integers(lo, hi + 1))


def _budgets(rng, B, N, extra=(), hi=None):
    """int32 [B]: unsorted, with duplicates; half from the edges (-3, 0, 1, N - 1, N, N + 1, extra), half random in 0 .. hi."""
    edges = [-3, 0, 1, N - 1, N, N + 1, *extra]
    hi = N + 1 if hi is None else hi
    return np.array([int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(0, hi + 1)) for _ in range(B)], dtype=np.int32)


def _votes(rng, seed, P, N, want_tokens):
    """pool [P, N] in 0 .. 1023, tokens [P, N] (>= 0) or None, synth's truth [P], the kind of pool."""
    dist = int(rng.integers(0, 6))
    a, t, tr = synth.fill(P, 1, N, 31_000 + seed, dist, want_tokens=True)
    pool, tok = np.ascontiguousarray(a[:, 0, :]), np.ascontiguousarray(t[:, 0, :])
    kind = f"D{dist}"
    fold = int(rng.choice([2, 3, 5, 40])) if rng.random() < 0.4 else 0
    if fold:                                                             # few bins: heavy ties
        pool, tr = pool % fold, (tr % fold).astype(np.int32)
    if seed % 20 == 7:                                                   # N distinct bins per row: code N - 1 in use, tie class N at k = N
        pool = np.stack([rng.choice(1024, size=N, replace=False) for _ in range(P)]).astype(np.int32)
        kind = "distinct"
    elif seed % 20 == 13:
        pool = np.repeat(rng.integers(0, 1024, size=(P, 1)), N, axis=1).astype(np.int32)
        kind = "single"
    if rng.random() < 0.3:                                               # samples of 0 tokens always fit
        tok = np.where(rng.random(tok.shape) < 0.25, 0, tok).astype(np.int32)
    return np.ascontiguousarray(pool.astype(np.int32)), (tok if want_tokens else None), tr.astype(np.int32), kind


def _truth(rng, pool, tr):
    """synth's own truth / a value of the row / a value absent from the row; on 30 % of the draws some rows outside or at the end of the bins."""
    P, N = pool.shape
    kind = str(rng.choice(["synth", "in_pool", "absent"]))
    if kind == "in_pool":
        tr = pool[np.arange(P), rng.integers(0, N, size=P)].copy()
    elif kind == "absent":
        tr = np.array([next(v for v in range(int(s), int(s) + 1024) if (v % 1024) not in row) % 1024
                       for s, row in zip(rng.integers(0, 1024, size=P), (set(r.tolist()) for r in pool))], dtype=np.int32)
    tr = tr.astype(np.int32)
    if rng.random() < 0.3:
        tr[:: int(rng.integers(1, 5))] = int(rng.choice(TRUTH_ODD))
    return tr, kind


def _token_budgets(rng, B, tok):
    """int64 [B]: 0, below the cheapest sample, a pool's whole cost, beyond it, 2^62, negative; half random."""
    total = tok.astype(np.int64).sum(axis=1)
    edges = [0, max(int(tok.min()) - 1, 0), int(total[0]), int(total.max()), int(total.max()) + 3, 2 ** 62, -5]
    return np.array([int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(0, int(total.max()) + 2)) for _ in range(B)], dtype=np.int64)


def _weights(rng, P, N):
    kind = str(rng.choice(["random", "equal", "few", "ones"]))
    if kind == "random":
        w = rng.integers(0, WEIGHT_MAX + 1, size=(P, N))
    elif kind == "equal":
        w = np.full((P, N), int(rng.choice([1, 77, WEIGHT_MAX])))
    elif kind == "few":
        w = rng.integers(0, 4, size=(P, N))                             # ties between weight sums, weights of 0
    else:
        w = np.ones((P, N), dtype=np.int64)
    if rng.random() < 0.4:
        w[rng.integers(0, P)] = 0                                        # a row without a mode
    if rng.random() < 0.4:
        w[rng.integers(0, P)] = WEIGHT_MAX                               # N x (2^24 - 1) < 2^32
    return np.ascontiguousarray(w.astype(np.int32)), kind


@lru_cache(maxsize=None)
def _beta(N: int, conf_pct: int):
    return adaptive.beta_rule(N, Fraction(conf_pct, 100))


def _rules(rng, B, N):
    """need int32 [B, N + 1], every row of its own kind: never / margin_rule / beta_rule / random (any int32 is legal: clamped on the device)."""
    rows, kinds = [], []
    for _ in range(B):
        k = str(rng.choice(["never", "margin", "beta", "random"]))
        if k == "never":
            row = adaptive.never(N)
        elif k == "margin":
            row = adaptive.margin_rule(N, int(rng.integers(1, 6)))
        elif k == "beta":
            row = _beta(N, int(rng.choice([90, 95])))
        else:
            row = rng.integers(-2, N + 4, size=N + 1).astype(np.int32)
        rows.append(row)
        kinds.append(k)
    return np.ascontiguousarray(np.stack(rows), dtype=np.int32), kinds


def draw(entry: str, seed: int, work_div: int = 1):
    """One valid call of ``entry``, deterministic in (entry, seed, work_div)."""
    rng = np.random.default_rng((STREAM[entry], int(seed)))
    c = SimpleNamespace(entry=entry, seed=int(seed))
    tight = entry != "expected" and rng.random() < 0.15
    N = int(rng.choice(N_EDGES[-4:])) if tight else (int(rng.choice(N_EDGES, p=N_EDGE_P)) if rng.random() < 0.5 else int(rng.integers(1, 257)))
    tight_b = tight and rng.random() < 0.5
    B = int(rng.choice(B_EDGES[-2:])) if tight_b else _pick(rng, B_EDGES, 0.4, 1, 32)
    c.N, c.B = N, B
    c.device = bool(rng.random() < 0.5)
    c.grid = int(rng.integers(1, 31)) if rng.random() < 0.2 else 0
    if entry == "expected":
        c.P = P = int(rng.integers(1, 7 if N <= 64 else 4))
        c.R, c.shuffled = 1, False
        c.pool, _, tr, c.pool_kind = _votes(rng, seed, P, N, False)
        c.truth, c.truth_kind = _truth(rng, c.pool, tr)
        c.n_valid = _budgets(rng, B, N)
        c.work = P * N
        return c
    c.shuffled = shuffled = entry not in HAS_ORDER or bool(rng.random() < 0.65)
    R = 1 if not shuffled else (int(rng.choice(R_EDGES[:3])) if tight and not tight_b else _pick(rng, R_EDGES, 0.5, 1, 600))
    # the budgets first: the longest walk bounds the lanes
    if entry == "iid":
        c.n_draws = _budgets(rng, B, N, extra=(2 * N, 255, 256, 257, 1000), hi=2 * N)
        if seed % 20 == 3:
            c.n_draws[int(rng.integers(0, B))] = 4096
        walk = max(int(c.n_draws.max()), 1)
    elif entry in ("resample", "weighted"):
        c.n_valid = _budgets(rng, B, N)
        walk = max(int(np.clip(c.n_valid, 0, N).max()), 1)
    elif entry == "adaptive":
        c.cap = _budgets(rng, B, N)
        walk = N
    else:
        walk = N
    lanes_max = max(1, WORK[entry] // work_div // walk)
    R = min(R, lanes_max)
    p_max = max(1, min(lanes_max // R, 700))
    how = "many" if tight and not tight_b else str(rng.choice(["few", "ragged", "many"], p=[0.4, 0.3, 0.3]))
    if how == "few":                                                     # fewer than 64 lanes (R allowing)
        P = int(rng.integers(1, max(1, 63 // R) + 1))
    elif how == "ragged":                                                # a few chunks, the last one partial
        P = int(rng.integers(1, max(1, 1000 // R) + 1))
        P += (P * R) % 64 == 0
    else:                                                                # several chunks; R <= 3: more rows than a chunk of lanes can touch
        P = int(rng.integers(max(1, min(300, p_max) if R <= 3 else p_max // 2), p_max + 1))
    c.P = P = max(1, min(P, p_max))
    c.R = R
    c.work = P * R * walk
    want_tokens = entry == "token_budget" or bool(rng.random() < 0.5)
    c.pool, c.tokens, tr, c.pool_kind = _votes(rng, seed, P, N, want_tokens)
    c.truth, c.truth_kind = _truth(rng, c.pool, tr)
    c.r_begin = int(rng.choice([0, 7, 2 ** 31 - 1 - R])) if shuffled else 0
    c.r_end = c.r_begin + R
    c.p_offset = int(rng.choice([0, 5, 2 ** 33]))
    c.vote_seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    c.M = (N + 1) if rng.random() < 0.5 else 0
    c.want_cells = entry in HAS_ORDER and not shuffled                   # pool order: cells, cell tokens and cell votes are asked for
    if entry == "token_budget":
        c.token_budgets = _token_budgets(rng, B, c.tokens)
    elif entry == "weighted":
        c.weights, c.weight_kind = _weights(rng, P, N)
        c.rule = int(rng.integers(0, 2))
    elif entry == "adaptive":
        c.need, c.rule_kinds = _rules(rng, B, N)
        c.rule_flags = None if rng.random() < 0.25 else rng.integers(0, 2, size=B).astype(np.int32)
    return c


BUDGET_FIELD = {"resample": "n_valid", "weighted": "n_valid", "iid": "n_draws", "adaptive": "cap", "expected": "n_valid"}


def budgets_of(c):
    """The per-budget sample counts of the case (a token budget counts tokens, not samples: None)."""
    return getattr(c, BUDGET_FIELD[c.entry]) if c.entry in BUDGET_FIELD else None


def describe(c) -> str:
    keys = ("entry", "seed", "N", "B", "P", "R", "shuffled", "device", "grid", "M", "r_begin", "p_offset", "pool_kind", "truth_kind", "work")
    return " ".join(f"{k}={getattr(c, k)}" for k in keys if hasattr(c, k))


# ---- the mirrors on a draw ---------------------------------------------------------------------------------------------------------------

def mirror(c, **over):
    """The entry's numpy mirror on the case (``over`` replaces fields: the wrong variants of the CPU test are built on it)."""
    a = SimpleNamespace(**{**vars(c), **over})
    r_end = a.r_end if a.shuffled else None
    M = a.M if a.M else None
    if a.entry == "resample":
        return resample.resample_prefix(a.pool, a.truth, a.n_valid, a.r_begin, a.r_end, a.vote_seed, tokens=a.tokens, p_offset=a.p_offset, M=M)
    if a.entry == "iid":
        return iid.iid_prefix(a.pool, a.truth, a.n_draws, a.r_begin, a.r_end, a.vote_seed, tokens=a.tokens, p_offset=a.p_offset, M=a.M)
    if a.entry == "token_budget":
        return token_budget.token_budget_prefix(a.pool, a.tokens, a.truth, a.token_budgets, a.r_begin, r_end, a.vote_seed, a.p_offset, M=M,
                                                want_cells=a.want_cells)
    if a.entry == "weighted":
        return weighted.weighted_prefix(a.pool, a.weights, a.truth, a.n_valid, a.rule, a.r_begin, r_end, a.vote_seed, a.p_offset, M=M,
                                        tokens=a.tokens, want_cells=a.want_cells)
    if a.entry == "adaptive":
        return adaptive.adaptive_prefix(a.pool, a.truth, a.cap, a.need, a.rule_flags, a.tokens, a.r_begin, r_end, a.vote_seed, a.p_offset, M=M,
                                        want_cells=a.want_cells)
    raise KeyError(a.entry)


def outputs_of(c, res) -> dict:
    """Every output the entry has for this case, by name, from a result object of the mirror or of a HOST-mode engine call."""
    out = {}
    for name in SUMMED + WRITTEN:
        v = getattr(res, name, None)
        if v is None or (name == "token_sum" and c.tokens is None) or (name == "per_resample" and not c.M):
            continue
        out[name] = v
    return out


def mirror_outputs(c, **over) -> dict:
    res = mirror(c, **over)
    assert res.error_bits == 0, (describe(c), res.error_bits)            # the draws are valid calls
    return outputs_of(c, res)


def same_outputs(got: dict, want: dict) -> bool:
    if set(got) != set(want):
        return False
    for k, w in want.items():
        if k == "cells":
            if not all(np.array_equal(got[k][f], w[f]) for f in CELL_FIELDS):
                return False
        elif not np.array_equal(got[k], w):
            return False
    return True
