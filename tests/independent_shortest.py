"""A second, deliberately naive implementation of scv_shortest_prefix_i32, written from the header text (include/scvote.h) alone: one Python
loop per (problem, ordering, budget), the first k samples of the ordering put through Python's ``sorted`` on the pair (tokens, pool index),
statistics.multimode over the votes of the first m.  It shares only the definition of the shuffle (resample.problem_streams / swap_index) with
the mirror in o1_inference_scaling_laws_amd/shortest.py."""
import statistics

import numpy as np

from o1_inference_scaling_laws_amd.resample import problem_streams, swap_index


def ordering(seed, pg, r, N):
    s = problem_streams(seed, [pg])[0]
    perm = list(range(N))
    for i in range(N - 1):
        j = int(swap_index(s, r, i, N))
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def kept(perm, toks, k, m):
    """V: the m elements of the first k of perm that come first by (tokens, pool index)."""
    return sorted(perm[:k], key=lambda x: (toks[x], x))[:m]


def shortest(pool, tokens, truth, n_valid, m_keep, r_begin, r_end, seed, p_offset, M, open_domain=False):
    """Returns a dict of the call's outputs; r_end None: pool order.  cells: {(p, b): (max_count, truth_count, n_modes, min_mode VALUE or -1,
    hit, spent)}."""
    P, N = pool.shape
    B = len(n_valid)
    shuffled = r_end is not None
    rs = list(range(r_begin, r_end)) if shuffled else [0]
    tie = np.zeros((B, 1025), dtype=np.int64)
    voted, spent, latency, tcs = (np.zeros(B, np.int64) for _ in range(4))
    per = np.zeros((len(rs), B, M), dtype=np.int64)
    cells = {}
    for p in range(P):
        row = [int(v) for v in pool[p].tolist()]
        if not open_domain:
            row = [v if 0 <= v < 1024 else 1023 for v in row]
        toks = [int(t) for t in tokens[p].tolist()]
        t = int(truth[p])
        t_ok = open_domain or 0 <= t < 1024
        for ri, r in enumerate(rs):
            perm = ordering(seed, p_offset + p, r, N) if shuffled else list(range(N))
            for b in range(B):
                k = min(max(int(n_valid[b]), 0), N)
                m = min(max(int(m_keep[b]), 0), k)
                V = kept(perm, toks, k, m)
                votes = [row[x] for x in V]
                modes = statistics.multimode(votes)
                hit = t_ok and t in modes
                if hit:
                    tie[b, len(modes)] += 1
                    if len(modes) < M:
                        per[ri, b, len(modes)] += 1
                tc = votes.count(t) if t_ok else 0
                v_tok = sum(toks[x] for x in V)
                t_m = toks[V[-1]] if V else 0
                s_tok = v_tok + (k - m) * t_m
                voted[b] += v_tok
                spent[b] += s_tok
                latency[b] += t_m
                tcs[b] += tc
                cells[(p, b)] = (max(votes.count(v) for v in votes) if votes else 0, tc, len(modes), min(modes) if modes else -1, int(hit), s_tok)
    return dict(tie=tie, voted=voted, spent=spent, latency=latency, truth_sum=tcs, per=per, cells=cells)
