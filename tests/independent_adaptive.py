"""A second, deliberately naive implementation of scv_adaptive_prefix_i32, written from the header text (include/scvote.h) alone: one Python
loop per (problem, ordering, rule), a collections.Counter over the samples counted so far, the counts SORTED at every step to read c1 and c2,
statistics.multimode over the samples at the stopping point.  It shares only the definition of the shuffle (resample.problem_streams /
swap_index) with the mirror in o1_inference_scaling_laws_amd/adaptive.py."""
import statistics
from collections import Counter

import numpy as np

from o1_inference_scaling_laws_amd.resample import problem_streams, swap_index


def ordering(seed, pg, r, N):
    s = problem_streams(seed, [pg])[0]
    perm = list(range(N))
    for i in range(N - 1):
        j = int(swap_index(s, r, i, N))
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def top_two(counter):
    """(c1, c2): the largest count, and the count of the second value in descending order of count (0 when there is only one value)."""
    counts = sorted(counter.values(), reverse=True)
    return counts[0], (counts[1] if len(counts) > 1 else 0)


def stopping_point(vals, n_max, need_row, flag, N):
    """the first n in 1 .. n_max at which the vote over vals[:n] stops; 0 when n_max is 0."""
    if n_max == 0:
        return 0
    seen = Counter()
    for n in range(1, n_max + 1):
        seen[vals[n - 1]] += 1
        c1, c2 = top_two(seen)
        if c1 >= min(max(int(need_row[c2]), 0), N + 1):
            return n
        if (flag & 1) and c1 - c2 > n_max - n:
            return n
        if n == n_max:
            return n
    raise AssertionError("unreachable")


def adaptive(pool, truth, cap, need, flags, tokens, r_begin, r_end, seed, p_offset, M):
    """Returns a dict of the call's outputs; r_end None: pool order.  cells: {(p, b): (max_count, truth_count, n_modes, min_mode, hit, tokens, votes)}."""
    P, N = pool.shape
    B = len(cap)
    shuffled = r_end is not None
    rs = list(range(r_begin, r_end)) if shuffled else [0]
    tie = np.zeros((B, 1025), dtype=np.int64)
    tsum, vsum, tcsum = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    hist = np.zeros((B, N + 1), dtype=np.int64)
    per = np.zeros((len(rs), B, M), dtype=np.int64)
    cells = {}
    for p in range(P):
        row = [v if 0 <= v < 1024 else 1023 for v in pool[p].tolist()]
        for ri, r in enumerate(rs):
            perm = ordering(seed, p_offset + p, r, N) if shuffled else list(range(N))
            vals = [row[x] for x in perm]
            for b in range(B):
                n_max = min(max(int(cap[b]), 0), N)
                n = stopping_point(vals, n_max, need[b], int(flags[b]), N)
                counted = vals[:n]
                modes = statistics.multimode(counted)
                t = int(truth[p])
                hit = 0 <= t < 1024 and t in modes
                if hit:
                    tie[b, len(modes)] += 1
                    if len(modes) < M:
                        per[ri, b, len(modes)] += 1
                tc = counted.count(t) if 0 <= t < 1024 else 0
                spent = sum(int(tokens[p, x]) for x in perm[:n]) if tokens is not None else 0
                tcsum[b] += tc
                tsum[b] += spent
                vsum[b] += n
                hist[b, n] += 1
                cells[(p, b)] = (max(Counter(counted).values()) if counted else 0, tc, len(modes), min(modes) if modes else -1, int(hit), spent, n)
    return dict(tie=tie, token_sum=tsum, vote_sum=vsum, truth_sum=tcsum, stop_hist=hist, per=per, cells=cells)
