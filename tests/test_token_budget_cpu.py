"""CPU tests of the token-budget mirror (o1_inference_scaling_laws_amd/token_budget.py, spec: scv_token_budget_prefix_i32 in
include/scvote.h): brute force with explicit prefixes and statistics.multimode, the reduction to resample_prefix when every sample costs
the same, and the curve helper's schema."""
import statistics

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import curves, resample, synth, token_budget
from o1_inference_scaling_laws_amd.resample import problem_streams, swap_index


def brute_perm(seed, pg, r, N):
    s = problem_streams(seed, [pg])[0]
    perm = list(range(N))
    for i in range(N - 1):
        j = int(swap_index(s, r, i, N))
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def brute(pool, tokens, truth, budgets, r_begin, r_end, seed, p_offset, M):
    """Every (problem, ordering, budget) by hand: walk the ordering until the next sample does not fit, multimode over the prefix."""
    P, N = pool.shape
    B = len(budgets)
    shuffled = r_end is not None
    rs = range(r_begin, r_end) if shuffled else [0]
    tie = np.zeros((B, 1025), dtype=np.int64)
    tsum, vsum, tcsum = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    per = np.zeros((len(rs), B, M), dtype=np.int64)
    cells = {}
    for p in range(P):
        vals = [v if 0 <= v < 1024 else 1023 for v in pool[p].tolist()]
        for ri, r in enumerate(rs):
            perm = brute_perm(seed, p_offset + p, r, N) if shuffled else list(range(N))
            for b, T in enumerate(budgets):
                spent, prefix = 0, []
                for x in perm:
                    if spent + int(tokens[p, x]) > T:
                        break
                    spent += int(tokens[p, x])
                    prefix.append(vals[x])
                modes = statistics.multimode(prefix) if prefix else []
                t = int(truth[p])
                hit = 0 <= t < 1024 and t in modes
                if hit:
                    tie[b, len(modes)] += 1
                    per[ri, b, len(modes)] += 1
                tc = prefix.count(t) if 0 <= t < 1024 else 0
                tsum[b] += spent
                vsum[b] += len(prefix)
                tcsum[b] += tc
                if not shuffled:
                    mx = max(prefix.count(m) for m in modes) if modes else 0
                    cells[(p, b)] = (mx, tc, len(modes), min(modes) if modes else -1, int(hit), spent)
    return tie, tsum, vsum, tcsum, per, cells


def random_case(rng):
    P = int(rng.integers(1, 4))
    N = int(rng.integers(1, 13))
    nvals = int(rng.integers(1, 5))
    pool = rng.integers(0, nvals, size=(P, N)) * 37
    if rng.random() < 0.2:
        pool[rng.random(pool.shape) < 0.2] = 2000                       # outside the bins: counts as 1023
    tokens = rng.integers(0, 50, size=(P, N))
    tokens[rng.random(tokens.shape) < 0.25] = 0                         # failed samples: (answer 0, tokens 0) still vote
    truth = rng.integers(0, nvals + 1, size=P) * 37
    if rng.random() < 0.1:
        truth[0] = 5000                                                 # outside the bins: never hits
    total = tokens.sum(axis=1).max()
    choices = [-5, -1, 0, int(tokens[:, 0].min()) - 1, int(total), int(total) + 3, 2 ** 31 + 7, 2 ** 40]
    B = int(rng.integers(1, 7))
    budgets = [int(rng.choice(choices)) if rng.random() < 0.5 else int(rng.integers(0, total + 2)) for _ in range(B)]
    return pool.astype(np.int32), tokens.astype(np.int32), truth.astype(np.int32), budgets


@pytest.mark.parametrize("shuffled", [False, True])
def test_mirror_equals_brute_force(shuffled):
    rng = np.random.default_rng(11 + shuffled)
    for case in range(150):
        pool, tokens, truth, budgets = random_case(rng)
        P, N = pool.shape
        M = N + 1
        if shuffled:
            r0 = int(rng.integers(0, 5))
            r1 = r0 + int(rng.integers(1, 4))
            seed, p_off = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 1 << 34))
        else:
            r0, r1, seed, p_off = 0, None, 0, 0
        got = token_budget.token_budget_prefix(pool, tokens, truth, budgets, r0, r1, seed, p_off, M=M, want_cells=not shuffled)
        tie, tsum, vsum, tcsum, per, cells = brute(pool, tokens, truth, budgets, r0, r1, seed, p_off, M)
        assert np.array_equal(got.tie_class_hits, tie), case
        assert np.array_equal(got.token_sum, tsum) and np.array_equal(got.vote_count_sum, vsum), case
        assert np.array_equal(got.truth_count_sum, tcsum) and np.array_equal(got.per_resample, per), case
        assert got.error_bits & ~1 == 0
        if not shuffled:
            for (p, b), want in cells.items():
                c = got.cells[p, b]
                assert (int(c["max_count"]), int(c["truth_count"]), int(c["n_modes"]), int(c["min_mode"]), int(c["hit"]),
                        int(got.cell_tokens[p, b])) == want, (case, p, b)
        assert (got.token_sum <= np.clip(np.array(budgets), 0, None) * got.P * got.R).all()


def test_orderings_are_those_of_resample():
    s = [brute_perm(9, 3 + p, r, 20) for p in range(2) for r in range(4, 7)]
    assert np.array_equal(token_budget.orderings(2, 20, 4, 7, 9, p_offset=3), np.array(s))


@pytest.mark.parametrize("dist", range(6))
def test_equal_tokens_reduce_to_resample_prefix(dist):
    """Every token t > 0 and T_b = n_b * t + delta_b (0 <= delta_b < t): the prefix is n_b long in every ordering."""
    rng = np.random.default_rng(dist)
    P, N, t = 4, 40, 7
    a, _, tr = synth.fill(P, 1, N, 30 + dist, dist)
    pool = a[:, 0, :].copy()
    tokens = np.full_like(pool, t)
    nb = np.array([0, 1, 2, 5, 17, 40, 40, 3], dtype=np.int64)
    budgets = nb * t + rng.integers(0, t, size=nb.shape)
    got = token_budget.token_budget_prefix(pool, tokens, tr, budgets, 3, 40, seed=5, p_offset=2, M=N + 1)
    want = resample.resample_prefix(pool, tr, nb.astype(np.int32), 3, 40, seed=5, tokens=tokens, p_offset=2, M=N + 1)
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
    assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
    assert np.array_equal(got.vote_count_sum, nb * P * 37)
    assert [got.exact_accuracy(b) for b in range(8)] == [want.exact_accuracy(b) for b in range(8)]
    assert got.avg_votes(4) == 17.0


def test_negative_tokens_and_class_overflow_set_their_bits():
    pool = np.tile(np.arange(8, dtype=np.int32), (2, 1))
    tokens = np.ones_like(pool)
    tr = np.array([0, 1], dtype=np.int32)
    assert token_budget.token_budget_prefix(pool, tokens, tr, [8], M=9).error_bits == 0
    assert token_budget.token_budget_prefix(pool, tokens, tr, [8], M=4).error_bits == resample.ERR_CLASS_BIT
    tokens[1, 3] = -1
    assert token_budget.token_budget_prefix(pool, tokens, tr, [8]).error_bits & token_budget.ERR_TOKEN_BIT


def test_mirror_rejects_shapes_outside_the_limits():
    pool = np.zeros((1, 4), dtype=np.int32)
    with pytest.raises(ValueError):
        token_budget.token_budget_prefix(np.zeros((1, 257), np.int32), np.zeros((1, 257), np.int32), [0], [1])
    with pytest.raises(ValueError):
        token_budget.token_budget_prefix(pool, pool, [0], np.ones(33))
    with pytest.raises(ValueError):
        token_budget.token_budget_prefix(pool, pool, [0], [1], r_begin=1)              # pool order is the one draw r = 0
    with pytest.raises(ValueError):
        token_budget.token_budget_prefix(pool, pool, [0], [1], 0, 2, want_cells=True)  # cells: pool order only


class _MirrorEngine:
    """The curve helper's engine interface, served by the CPU mirror."""
    def token_budget_prefix(self, pool, tokens, truth, token_budgets, resamples=None, seed=0, r_begin=0, p_offset=0, M=None,
                            want_cells=False):
        r_end = None if resamples is None else r_begin + resamples
        return token_budget.token_budget_prefix(pool, tokens, truth, token_budgets, r_begin, r_end, seed, p_offset,
                                                M=None if not M else M, want_cells=want_cells)


@pytest.mark.parametrize("resamples", [None, 6])
def test_token_budget_records_spend_at_most_the_limit(resamples):
    a, t, tr = synth.fill(6, 1, 128, 2, 1, want_tokens=True)
    limits = [2 ** i for i in range(11, 19)] + [2 ** 22]
    recs = curves.token_budget_records(_MirrorEngine(), a[:, 0, :], tr, t[:, 0, :], limits, resamples=resamples, seed=3)
    assert [r["token_limit"] for r in recs] == limits
    assert all(set(r) == {"token_limit", "accuracy", "avg_tokens_used"} for r in recs)
    used = [r["avg_tokens_used"] for r in recs]
    assert all(u <= lim for u, lim in zip(used, limits)) and used == sorted(used)
    assert all(0.0 <= r["accuracy"] <= 1.0 and isinstance(r["avg_tokens_used"], float) for r in recs)
    assert used[-1] == float(np.float64(int(t[:, 0, :].astype(np.int64).sum())) / 6)        # 2^22 holds every pool whole
