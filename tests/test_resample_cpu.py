"""CPU tests of the resampled majority vote (include/scvote.h scv_resample_prefix_i32): the numpy mirror against a scalar
restatement of the header text, unbiasedness against exact enumeration, slicing / sharding, the n_valid = N identity, and the
curve records.  No GPU."""
import itertools
import math
import statistics
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import curves, resample, synth
from o1_inference_scaling_laws_amd.scoring import accuracy_from_tie_classes

MASK64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix64_int(z):
    z &= MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def scalar_reference(pool, truth, n_valid, r_begin, r_end, seed, tokens=None, p_offset=0, M=None):
    """The header text, one cell at a time: Fisher-Yates + statistics.multimode in plain Python ints."""
    P, N = len(pool), len(pool[0])
    B = len(n_valid)
    tie = [[0] * 1025 for _ in range(B)]
    tsum, tcsum = [0] * B, [0] * B
    per = [[[0] * M for _ in range(B)] for _ in range(r_end - r_begin)] if M else None
    err = 0
    for p in range(P):
        pg = p_offset + p
        s = mix64_int(((seed ^ 0xD6E8FEB86659FD93) + G * (pg + 1)) & MASK64)
        row = []
        for v in pool[p]:
            v = int(v)
            if not 0 <= v <= 1023:
                err |= 1
                v = 1023
            row.append(v)
        t = int(truth[p])
        for r in range(r_begin, r_end):
            perm = list(range(N))
            for i in range(N - 1):
                u = mix64_int(s + G * (r * N + i + 1))
                j = i + (((u >> 32) * (N - i)) >> 32)
                perm[i], perm[j] = perm[j], perm[i]
            for b in range(B):
                k = min(max(int(n_valid[b]), 0), N)
                sub = [row[x] for x in perm[:k]]
                if tokens is not None:
                    tsum[b] += sum(int(tokens[p][x]) for x in perm[:k])
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


def small_pool(rng, P, N, values):
    return rng.integers(0, values, size=(P, N)).astype(np.int32)


@pytest.mark.parametrize("case", range(8))
def test_mirror_equals_scalar_restatement(case):
    rng = np.random.default_rng(100 + case)
    P = int(rng.integers(1, 4))
    N = [1, 2, 3, 5, 7, 8, 12, 17][case]
    pool = small_pool(rng, P, N, int(rng.integers(2, 6)))                  # few distinct values: ties everywhere
    truth = rng.integers(0, 6, size=P).astype(np.int32)
    if case % 3 == 1:                                                      # out-of-domain votes (clamped to bin 1023; flagged)
        pool[0, 0] = -7
        pool[-1, -1] = 5000
        truth[0] = 1023
    if case % 4 == 2:
        truth[-1] = 2000                                                  # a truth outside the bins never hits
    nv = np.array([0, N + 3, 1, N, max(N // 2, 1), 1, -2][: 2 + case % 6], dtype=np.int32)   # 0, > N, duplicates, unsorted, negative
    rng.shuffle(nv)
    tokens = rng.integers(100, 12000, size=(P, N)).astype(np.int32) if case % 2 == 0 else None
    r0, r1 = [(0, 5), (3, 9), (7, 8), (0, 1)][case % 4]
    M = 3 if case == 5 else 8
    got = resample.resample_prefix(pool, truth, nv, r0, r1, seed=1234 + case, tokens=tokens, p_offset=case * 11, M=M)
    tie, tsum, tcsum, per, err = scalar_reference(pool.tolist(), truth.tolist(), nv.tolist(), r0, r1, 1234 + case,
                                                  tokens=None if tokens is None else tokens.tolist(), p_offset=case * 11, M=M)
    assert np.array_equal(got.tie_class_hits, tie)
    assert np.array_equal(got.truth_count_sum, tcsum)
    assert np.array_equal(got.per_resample, per)
    if tokens is not None:
        assert np.array_equal(got.token_sum, tsum)
    assert got.error_bits == err


def test_swap_indices_follow_the_header_formula():
    s = resample.problem_streams(77, np.arange(5))
    for p in range(5):
        want = mix64_int((77 ^ 0xD6E8FEB86659FD93) + G * (p + 1))
        assert int(s[p]) == want
        for r in (0, 3, 2 ** 31 - 1):
            for i in (0, 5, 9):
                u = mix64_int(want + G * (r * 10 + i + 1))
                assert int(resample.swap_index(s[p], r, i, 10)) == i + (((u >> 32) * (10 - i)) >> 32)


def exact_expected_score(row, truth, k):
    """E[score] of the majority vote over a uniformly random k-subset, by enumerating all C(N, k) subsets."""
    total, n = Fraction(0), 0
    for sub in itertools.combinations(range(len(row)), k):
        n += 1
        if k == 0:
            continue
        modes = statistics.multimode([row[i] for i in sub])
        if truth in modes:
            total += Fraction(1, len(modes))
    return total / n


def test_estimator_is_unbiased():
    rng = np.random.default_rng(5)
    P, N, R = 3, 9, 20000
    pool = small_pool(rng, P, N, 4)
    truth = pool[:, 0].copy()
    nv = np.arange(1, N + 1, dtype=np.int32)
    res = resample.resample_prefix(pool, truth, nv, 0, R, seed=99, M=N + 1)
    for b, k in enumerate(nv):
        exact = sum(exact_expected_score(pool[p].tolist(), int(truth[p]), int(k)) for p in range(P)) / P
        per_cell = res.resample_accuracy(b)                                  # [R]: the mean score of each ordering
        assert math.isclose(float(per_cell.mean()), res.accuracy(b), rel_tol=1e-12, abs_tol=1e-15)
        se = max(float(per_cell.std(ddof=1)) / math.sqrt(R), 1e-12)               # standard error of the mean over orderings
        assert abs(res.accuracy(b) - float(exact)) <= 4 * se + 1e-12, (int(k), res.accuracy(b), float(exact), se)
    assert res.exact_accuracy(N - 1) == sum(exact_expected_score(pool[p].tolist(), int(truth[p]), N) for p in range(P)) / P


def test_slices_and_shards_add_up():
    a, t, tr = synth.fill(7, 1, 24, 3, 1, want_tokens=True)
    pool, tok = a[:, 0, :], t[:, 0, :]
    nv = np.array([1, 2, 4, 8, 16, 24, 5], dtype=np.int32)
    whole = resample.resample_prefix(pool, tr, nv, 0, 40, seed=8, tokens=tok, M=25)
    s1 = resample.resample_prefix(pool, tr, nv, 0, 13, seed=8, tokens=tok, M=25)
    s2 = resample.resample_prefix(pool, tr, nv, 13, 40, seed=8, tokens=tok, M=25)
    for f in ("tie_class_hits", "token_sum", "truth_count_sum"):
        assert np.array_equal(getattr(whole, f), getattr(s1, f) + getattr(s2, f)), f
    assert np.array_equal(whole.per_resample, np.concatenate([s1.per_resample, s2.per_resample]))
    h1 = resample.resample_prefix(pool[:3], tr[:3], nv, 0, 40, seed=8, tokens=tok[:3], M=25)
    h2 = resample.resample_prefix(pool[3:], tr[3:], nv, 0, 40, seed=8, tokens=tok[3:], p_offset=3, M=25)
    for f in ("tie_class_hits", "token_sum", "truth_count_sum", "per_resample"):
        assert np.array_equal(getattr(whole, f), getattr(h1, f) + getattr(h2, f)), f


def prefix_counters(pool, truth, n_valid, tokens=None):
    """The existing prefix semantics (scv_aggregate_prefix_i32) on the unpermuted pool, by statistics.multimode."""
    P, N = pool.shape
    B = len(n_valid)
    tie = np.zeros((B, 1025), dtype=np.int64)
    ts, tcs = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for p in range(P):
        for b, n in enumerate(n_valid):
            k = min(max(int(n), 0), N)
            sub = pool[p, :k].tolist()
            tcs[b] += sub.count(int(truth[p]))
            if tokens is not None:
                ts[b] += int(tokens[p, :k].sum())
            if sub:
                modes = statistics.multimode(sub)
                if int(truth[p]) in modes:
                    tie[b, len(modes)] += 1
    return tie, ts, tcs


@pytest.mark.parametrize("dist", [0, 1, 3])
def test_whole_pool_budgets_equal_R_times_the_prefix_result(dist):
    a, t, tr = synth.fill(6, 1, 30, 17, dist, want_tokens=True)
    pool, tok = a[:, 0, :], t[:, 0, :]
    nv = np.array([30, 30, 99], dtype=np.int32)
    R = 11
    res = resample.resample_prefix(pool, tr, nv, 4, 4 + R, seed=3, tokens=tok)
    tie, ts, tcs = prefix_counters(pool, tr, nv, tok)
    assert np.array_equal(res.tie_class_hits, R * tie)
    assert np.array_equal(res.token_sum, R * ts)
    assert np.array_equal(res.truth_count_sum, R * tcs)
    assert res.accuracy(0) == accuracy_from_tie_classes(tie[0], 6)


def test_class_overflow_sets_bit_1_and_drops_nothing_silently():
    pool = np.array([[1, 2, 3, 4]], dtype=np.int32)                       # every subset is an all-way tie
    res = resample.resample_prefix(pool, np.array([1], dtype=np.int32), np.array([4], dtype=np.int32), 0, 3, seed=1, M=2)
    assert res.error_bits & 2
    assert res.tie_class_hits[0, 4] == 3


class _MirrorEngine:
    """The curve helper's engine interface, served by the CPU mirror."""
    def resample_prefix(self, pool, truth, n_valid, resamples, seed, tokens=None, r_begin=0, p_offset=0, M=None):
        return resample.resample_prefix(pool, truth, n_valid, r_begin, r_begin + resamples, seed, tokens=tokens, p_offset=p_offset,
                                        M=None if not M else M)


def test_expected_majority_records_have_the_reference_schema():
    a, t, tr = synth.fill(5, 1, 128, 2, 1, want_tokens=True)
    limits = [2 ** i for i in range(11, 19)]
    recs = curves.expected_majority_records(_MirrorEngine(), a[:, 0, :], tr, t[:, 0, :], limits, resamples=4, seed=1)
    assert [r["token_limit"] for r in recs] == limits
    assert all(set(r) == {"token_limit", "accuracy", "avg_tokens_used"} for r in recs)
    assert all(0.0 <= r["accuracy"] <= 1.0 and isinstance(r["avg_tokens_used"], float) for r in recs)
    # avg tokens grow with the number of samples; the whole-pool point is the pool's mean token total
    assert recs[-1]["avg_tokens_used"] == float(np.float64(int(t[:, 0, :].astype(np.int64).sum())) / 5)
    assert [(t_, n) for t_, n in curves.resampled_budgets(shade_regions=True)] == [(2 ** i, 2 ** (i - 11)) for i in range(11, 19)]
    with pytest.raises(ValueError):
        curves.resampled_budgets([1024])


def test_mirror_rejects_shapes_outside_the_limits():
    pool = np.zeros((1, 257), dtype=np.int32)
    with pytest.raises(ValueError):
        resample.resample_prefix(pool, [0], [1], 0, 1, 0)
    with pytest.raises(ValueError):
        resample.resample_prefix(pool[:, :4], [0], np.ones(33, dtype=np.int32), 0, 1, 0)
    with pytest.raises(ValueError):
        resample.resample_prefix(pool[:, :4], [0], [1], 3, 2, 0)
