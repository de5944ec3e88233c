"""Naive statement of scv_iid_prefix_i32, written from the text of include/scvote.h alone: one pure-Python loop per (problem, resample,
budget), statistics.multimode on the drawn values, a scalar mix64.  Shares no code with o1_inference_scaling_laws_amd/iid.py.

    s      = mix64((seed ^ 0xA0761D6478BD642F) + G * (pg + 1))
    draw i: u = mix64(s + G * (r * 65536 + i + 1)),  x_i = pool[p, mulhi32(hi32(u), N)]
    cell (p, r, b) = statistics.multimode(x_0 ... x_{k_b - 1}),  k_b = max(n_draws[b], 0)
"""
import statistics

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SALT = 0xA0761D6478BD642F
NUM_BINS, TIE_CLASSES = 1024, 1025


def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_counter(r, i):
    return r * 65536 + i + 1


def draws(pool_row, seed, pg, r, k):
    N = len(pool_row)
    s = mix64((seed ^ SALT) + G * (pg + 1))
    out = []
    for i in range(k):
        u = mix64(s + G * draw_counter(r, i))
        out.append(((u >> 32) * N) >> 32)
    return out


def iid_prefix(pool, truth, n_draws, r_begin, r_end, seed, tokens=None, p_offset=0, M=0):
    """Returns (tie [B][1025], token_sum [B], truth_count_sum [B], per_resample [R][B][M] or None, error bits) as Python lists."""
    P, B, R = len(pool), len(n_draws), r_end - r_begin
    tie = [[0] * TIE_CLASSES for _ in range(B)]
    tsum, tcsum = [0] * B, [0] * B
    per = [[[0] * M for _ in range(B)] for _ in range(R)] if M else None
    err = 0
    for p in range(P):
        row = []
        for v in pool[p]:
            v = int(v)
            if not 0 <= v < NUM_BINS:
                err |= 1
                v = NUM_BINS - 1
            row.append(v)
        t = int(truth[p])
        for r in range(r_begin, r_end):
            for b in range(B):
                k = max(int(n_draws[b]), 0)
                idx = draws(row, seed, p_offset + p, r, k)
                xs = [row[j] for j in idx]
                if tokens is not None:
                    tsum[b] += sum(int(tokens[p][j]) for j in idx)
                if 0 <= t < NUM_BINS:
                    tcsum[b] += xs.count(t)
                if not xs:
                    continue
                modes = statistics.multimode(xs)
                if 0 <= t < NUM_BINS and t in modes:
                    tie[b][len(modes)] += 1
                    if per is not None:
                        if len(modes) < M:
                            per[r - r_begin][b][len(modes)] += 1
                        else:
                            err |= 2
    return tie, tsum, tcsum, per, err
