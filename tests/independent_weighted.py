"""A SECOND implementation of the weighted majority vote / best-of-N of scv_weighted_prefix_i32, written from the TEXT of include/scvote.h
alone: pure Python, one prefix at a time, dicts keyed by the vote's value, Fraction scores.  No dense codes, no tables, no running rule --
the mirror (o1_inference_scaling_laws_amd/weighted.py) and the HIP kernel are the other two readings.  The shuffle is written out here from
the header's lines on scv_resample_prefix_i32 (s, u, j, swap), with Python integers; the splitmix64 finaliser is Steele, Lea & Flood 2014 /
Vigna's public-domain splitmix64.c.  Test infrastructure: only tests/ import it."""
from __future__ import annotations

from fractions import Fraction

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SALT = 0xD6E8FEB86659FD93
BINS = 1024
WEIGHT_MAX = (1 << 24) - 1


def mix64(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def permutation(seed: int, pg: int, r: int, N: int) -> list:
    s = mix64((seed ^ SALT) + G * (pg + 1))
    perm = list(range(N))
    for i in range(N - 1):
        u = mix64(s + G * (r * N + i + 1))
        j = i + (((u >> 32) * (N - i)) >> 32)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def prefix_cell(votes, weights, truth: int, rule: int):
    """(top W, W(truth), n_modes, min_mode, hit, score) of one prefix.  Votes outside the bins count as value 1023."""
    W = {}
    for v, w in zip(votes, weights):
        v = v if 0 <= v < BINS else BINS - 1
        W[v] = W.get(v, 0) + w if rule == 0 else max(W.get(v, 0), w)
    top = max(W.values(), default=0)
    if top <= 0:
        return 0, W.get(truth, 0) if 0 <= truth < BINS else 0, 0, -1, False, Fraction(0)
    modes = sorted(v for v, x in W.items() if x == top)
    tw = W.get(truth, 0) if 0 <= truth < BINS else 0
    hit = 0 <= truth < BINS and truth in modes
    return top, tw, len(modes), modes[0], hit, Fraction(1, len(modes)) if hit else Fraction(0)


def weighted_prefix(pool, weights, truth, n_valid, rule, r_begin=0, r_end=None, seed=0, p_offset=0, tokens=None, per_out=None,
                    cell_tokens_out=None):
    """Returns (tie[b] = {n_modes: hits}, score_sum[b] (Fraction), token_sum[b], cells[p][b] (pool order only, else None)).
    ``per_out``: a caller's [R][B][M] lists of zeros, filled with the hits of every ordering by n_modes (< M).  ``cell_tokens_out``: a
    caller's [P][B] lists, filled with the tokens of every prefix (pool order, with tokens)."""
    P, N = len(pool), len(pool[0])
    B = len(n_valid)
    shuffled = r_end is not None
    rs = range(r_begin, r_end) if shuffled else [None]
    tie = [dict() for _ in range(B)]
    score = [Fraction(0) for _ in range(B)]
    toks = [0] * B
    cells = None if shuffled else [[None] * B for _ in range(P)]
    for p in range(P):
        for ri, r in enumerate(rs):
            pi = permutation(seed, p_offset + p, r, N) if shuffled else list(range(N))
            for b in range(B):
                k = min(max(int(n_valid[b]), 0), N)
                idx = pi[:k]
                top, tw, nm, mm, hit, sc = prefix_cell([int(pool[p][i]) for i in idx], [int(weights[p][i]) for i in idx], int(truth[p]), rule)
                if hit:
                    tie[b][nm] = tie[b].get(nm, 0) + 1
                    if per_out is not None and nm < len(per_out[ri][b]):
                        per_out[ri][b][nm] += 1
                score[b] += sc
                if tokens is not None:
                    toks[b] += sum(int(tokens[p][i]) for i in idx)
                    if cell_tokens_out is not None:
                        cell_tokens_out[p][b] = sum(int(tokens[p][i]) for i in idx)
                if cells is not None:
                    cells[p][b] = (top, tw, nm, mm, int(hit))
    return tie, score, toks, cells
