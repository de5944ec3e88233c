"""scv_token_budget_wide_i32 one cell at a time, written from the text of include/scvote.h alone: Python integers, ``sorted(range(N), key=w)``, a
running sum that stops at the first sample that does not fit, and statistics.multimode.  Shares no code with
o1_inference_scaling_laws_amd/wide_budget.py or wide.py (the splitmix64 finaliser is Steele, Lea & Flood 2014)."""
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
    s = mix64_int(((seed ^ SALT) + G * (pg + 1)) & MASK64)
    w = [(mix64_int(s + G * (r * 4096 + i + 1)) & ~4095 & MASK64) | i for i in range(N)]
    return sorted(range(N), key=lambda i: w[i])


def naive_wide_budget(pool, tokens, truth, budgets, r_begin=0, r_end=None, seed=0, p_offset=0, M=None, open_domain=False):
    """r_end None: pool order.  Returns a dict: tie [B, 1025], token / vote / truth-count sums [B], per [R, B, M] or None, err, and in pool order
    cells (a list of P lists of B tuples (max_count, truth_count, n_modes, min_mode VALUE or -1, hit)) and cell_tokens [P][B]."""
    P, N, B = len(pool), len(pool[0]), len(budgets)
    shuffled = r_end is not None
    rs = range(r_begin, r_end) if shuffled else [0]
    tie = [[0] * 1025 for _ in range(B)]
    tsum, vsum, tcsum = [0] * B, [0] * B, [0] * B
    per = [[[0] * M for _ in range(B)] for _ in rs] if M else None
    cells = [[None] * B for _ in range(P)]
    ctok = [[0] * B for _ in range(P)]
    err = 0
    for p in range(P):
        row = []
        for v in pool[p]:
            v = int(v)
            if not open_domain and not 0 <= v <= 1023:
                err |= 1
                v = 1023
            row.append(v)
        t = int(truth[p])
        if not open_domain and not 0 <= t <= 1023:
            t = None                                                     # a truth outside the bins never hits
        toks = []
        for x in tokens[p]:
            x = int(x)
            if x < 0:
                err |= 16
                x = 0
            toks.append(x)
        for j, r in enumerate(rs):
            order = ordering(seed, p_offset + p, r, N) if shuffled else list(range(N))
            for b in range(B):
                T = int(budgets[b])
                n = spent = 0
                while n < N and spent + toks[order[n]] <= T:             # voting stops at the first sample that does not fit
                    spent += toks[order[n]]
                    n += 1
                if T < 0:
                    assert n == 0
                sub = [row[x] for x in order[:n]]
                tsum[b] += spent
                vsum[b] += n
                tc = sub.count(t) if t is not None else 0
                tcsum[b] += tc
                if not sub:
                    cells[p][b] = (0, 0, 0, -1, 0)
                    continue
                modes = statistics.multimode(sub)
                hit = t is not None and t in modes
                cells[p][b] = (sub.count(modes[0]), tc, len(modes), min(modes), int(hit))
                ctok[p][b] = spent
                if hit:
                    if len(modes) >= 1025:
                        err |= 2                                         # no column: counted in neither table
                        continue
                    tie[b][len(modes)] += 1
                    if M:
                        if len(modes) < M:
                            per[j][b][len(modes)] += 1
                        else:
                            err |= 2
    return {"tie": np.array(tie, dtype=np.int64), "token_sum": np.array(tsum, dtype=np.int64), "vote_count_sum": np.array(vsum, dtype=np.int64),
            "truth_count_sum": np.array(tcsum, dtype=np.int64), "per": np.array(per, dtype=np.int64) if M else None, "err": err,
            "cells": cells, "cell_tokens": np.array(ctok, dtype=np.int64)}
