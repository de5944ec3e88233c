"""scv_resample_wide_i32 one cell at a time, written from the text of include/scvote.h alone: Python integers, ``sorted`` and
statistics.multimode.  Shares no code with o1_inference_scaling_laws_amd/wide.py (the splitmix64 finaliser is Steele, Lea & Flood 2014)."""
import statistics

import numpy as np

MASK64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SALT = 0x8EBC6AF09C88C6E3


def mix64_int(z):
    z &= MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def ordering(seed, pg, r, N):
    """order of problem pg, resample r: the pool indices sorted ascending by w_i = (u_i & ~4095) | i."""
    s = mix64_int(((seed ^ SALT) + G * (pg + 1)) & MASK64)
    words = []
    for i in range(N):
        u = mix64_int(s + G * (r * 4096 + i + 1))
        words.append((u & ~4095 & MASK64) | i)
    assert len(set(words)) == N                                       # the index below the random bits makes them distinct
    return [w & 4095 for w in sorted(words)]


def naive_wide(pool, truth, n_valid, r_begin, r_end, seed, tokens=None, p_offset=0, M=None):
    """(tie int64 [B, 1025], token sums [B], truth-count sums [B], per_resample [R, B, M] or None, error bits)."""
    P, N = len(pool), len(pool[0])
    B = len(n_valid)
    tie = [[0] * 1025 for _ in range(B)]
    tsum, tcsum = [0] * B, [0] * B
    per = [[[0] * M for _ in range(B)] for _ in range(r_end - r_begin)] if M else None
    err = 0
    for p in range(P):
        row = []
        for v in pool[p]:
            v = int(v)
            if not 0 <= v <= 1023:
                err |= 1
                v = 1023
            row.append(v)
        t = int(truth[p])
        for r in range(r_begin, r_end):
            order = ordering(seed, p_offset + p, r, N)
            for b in range(B):
                k = min(max(int(n_valid[b]), 0), N)
                sub = [row[x] for x in order[:k]]
                if tokens is not None:
                    tsum[b] += sum(int(tokens[p][x]) for x in order[:k])
                tcsum[b] += sub.count(t)
                if not sub:
                    continue
                modes = statistics.multimode(sub)
                if t in modes:
                    tie[b][len(modes)] += 1
                    if M:
                        if len(modes) < M:
                            per[r - r_begin][b][len(modes)] += 1
                        else:
                            err |= 2
    return np.array(tie, dtype=np.int64), np.array(tsum, dtype=np.int64), np.array(tcsum, dtype=np.int64), \
        (np.array(per, dtype=np.int64) if M else None), err
