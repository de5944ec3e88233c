"""CPU tests of the resampled majority vote over wide pools (include/scvote.h scv_resample_wide_i32): the numpy mirror
(o1_inference_scaling_laws_amd/wide.py) against a naive restatement of the header text (tests/independent_wide.py), permutations, slicing /
sharding, error bits, the k = N identity against resample.py, the exact expectation, and the curve records.  No GPU."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import curves, expected, resample, synth, wide
from tests import independent_wide as ind


def pool_of(P, N, seed, dist, tokens=True):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=tokens)
    return a[:, 0, :].copy(), (t[:, 0, :].copy() if tokens else None), tr


def same(res, naive, tokens=True):
    tie, tsum, tcsum, per, err = naive
    assert np.array_equal(res.tie_class_hits, tie)
    assert np.array_equal(res.truth_count_sum, tcsum)
    if tokens:
        assert np.array_equal(res.token_sum, tsum)
    if per is not None:
        assert np.array_equal(res.per_resample, per)
    assert res.error_bits == err


CASES = [  # (P, N, R, r_begin, p_offset, dist, fold, budgets)
    (3, 1, 4, 0, 0, 1, 0, [1, 0, 2]),
    (2, 2, 5, 7, 5, 0, 2, [2, 1, 1, -1]),
    (3, 7, 6, 0, 1 << 33, 3, 0, [7, 3, 0, 9, 4]),
    (2, 65, 3, 2 ** 31 - 1 - 3, 0, 4, 3, [1, 2, 4, 8, 16, 32, 64, 65]),
    (2, 300, 2, 1, 2, 1, 0, [300, 1, 150, 256, 257]),
    (1, 1025, 2, 0, 0, 0, 5, [1025, 1024, 513, 3]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_mirror_equals_the_naive_restatement(case):
    P, N, R, r0, p_off, dist, fold, nv = CASES[case]
    pool, tok, tr = pool_of(P, N, 70 + case, dist)
    if fold:
        pool, tr = pool % fold, (tr % fold).astype(np.int32)
    if case % 2:
        tr[0] = (1023, -3, 2000)[case % 3]
    M = min(max(nv), N) + 1
    res = wide.resample_wide(pool, tr, nv, r0, r0 + R, seed=900 + case, tokens=tok, p_offset=p_off, M=M)
    same(res, ind.naive_wide(pool.tolist(), tr.tolist(), nv, r0, r0 + R, 900 + case, tokens=tok.tolist(), p_offset=p_off, M=M))


def test_every_order_is_a_permutation_and_prefixes_are_nested():
    for N in (1, 2, 3, 64, 1000, 4096):
        rs = np.array([0, 1, 77, 2 ** 31 - 2])
        order = wide.orderings(5, 2 ** 33 + 1, rs, N)
        assert order.shape == (4, N)
        assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(N), (4, 1)))
        for j, r in enumerate(rs[:2] if N > 64 else rs):
            assert order[j].tolist() == ind.ordering(5, 2 ** 33 + 1, int(r), N)
    a, b = wide.orderings(5, 0, [3], 500)[0], wide.orderings(5, 0, [4], 500)[0]
    assert not np.array_equal(a, b)
    assert not np.array_equal(a, wide.orderings(6, 0, [3], 500)[0]) and not np.array_equal(a, wide.orderings(5, 1, [3], 500)[0])


def test_slices_of_r_and_shards_of_p_add_up():
    pool, tok, tr = pool_of(7, 333, 9, 4)
    nv = np.array([333, 1, 64, 7, 200], dtype=np.int32)
    whole = wide.resample_wide(pool, tr, nv, 3, 43, seed=11, tokens=tok, M=334)
    parts = [wide.resample_wide(pool, tr, nv, lo, hi, seed=11, tokens=tok, M=334) for lo, hi in ((3, 10), (10, 43))]
    assert np.array_equal(sum(x.tie_class_hits for x in parts), whole.tie_class_hits)
    assert np.array_equal(sum(x.token_sum for x in parts), whole.token_sum)
    assert np.array_equal(sum(x.truth_count_sum for x in parts), whole.truth_count_sum)
    assert np.array_equal(np.concatenate([x.per_resample for x in parts]), whole.per_resample)
    shards = [wide.resample_wide(pool[lo:hi], tr[lo:hi], nv, 3, 43, seed=11, tokens=tok[lo:hi], p_offset=lo, M=334) for lo, hi in ((0, 3), (3, 7))]
    assert np.array_equal(sum(x.tie_class_hits for x in shards), whole.tie_class_hits)
    assert np.array_equal(sum(x.token_sum for x in shards), whole.token_sum)
    assert np.array_equal(sum(x.truth_count_sum for x in shards), whole.truth_count_sum)
    assert np.array_equal(sum(x.per_resample for x in shards), whole.per_resample)


def test_error_bits_and_bad_shapes():
    pool, _, tr = pool_of(3, 20, 21, 3, False)
    nv = [1, 5, 20]
    assert wide.resample_wide(pool, tr, nv, 0, 4, seed=1).error_bits == 0
    bad = pool.copy()
    bad[1, 3], bad[2, 0] = -1, 4096
    res = wide.resample_wide(bad, tr, nv, 0, 4, seed=1, M=21)
    assert res.error_bits == 1
    same(res, ind.naive_wide(bad.tolist(), tr.tolist(), nv, 0, 4, 1, M=21), tokens=False)
    ties = np.tile(np.arange(8, dtype=np.int32), (3, 1))                 # every prefix is an all-way tie: n_modes == k
    res = wide.resample_wide(ties, np.array([0, 1, 2]), [8], 0, 5, seed=1, M=8)
    assert res.error_bits == 2 and int(res.tie_class_hits[0, 8]) == 15 and int(res.per_resample.sum()) == 0
    assert wide.resample_wide(ties, np.array([0, 1, 2]), [8], 0, 5, seed=1, M=9).error_bits == 0
    for kw in (dict(pool=np.zeros((2, 4097), dtype=np.int32)), dict(pool=np.zeros((2, 0), dtype=np.int32)), dict(nv=[1] * 33), dict(r=(5, 4)),
               dict(r=(0, 2 ** 31)), dict(M=0)):
        r = kw.get("r", (0, 2))
        with pytest.raises(ValueError):
            wide.resample_wide(kw.get("pool", np.zeros((2, 8), dtype=np.int32)), np.zeros(2), kw.get("nv", [1]), r[0], r[1], seed=1, M=kw.get("M"))


@pytest.mark.parametrize("N", [1, 17, 256])
def test_whole_pool_budgets_equal_resample_prefix(N):
    """At k = N the ordering cannot matter: every output equals resample.resample_prefix at k = N on the same pool."""
    pool, tok, tr = pool_of(6, N, 13, 1)
    nv = [N, N + 3]
    got = wide.resample_wide(pool, tr, nv, 5, 14, seed=3, tokens=tok, M=N + 1)
    ref = resample.resample_prefix(pool, tr, nv, 5, 14, seed=3, tokens=tok, M=N + 1)
    assert np.array_equal(got.tie_class_hits, ref.tie_class_hits) and np.array_equal(got.per_resample, ref.per_resample)
    assert np.array_equal(got.token_sum, ref.token_sum) and np.array_equal(got.truth_count_sum, ref.truth_count_sum)


def test_against_the_exact_expectation():
    """Pool synth.fill(6, 1, 12, 7, 1), seed 11, R = 4000, budgets 1, 3, 6, 12: the mirror's accuracy within 5 sigma of the mean of
    expected.expected_majority_exact.  A cell's score lies in [0, 1], so its standard deviation is at most 0.5 and that of the mean over
    P * R cells at most 0.5 / sqrt(P * R): the bound is 5 * 0.5 / sqrt(6 * 4000) = 0.0161.  (Deviations seen: 0.0043 / 0.0029 / 0.0025 / 0.)"""
    P, R = 6, 4000
    pool, _, tr = pool_of(P, 12, 7, 1, False)
    nv = [1, 3, 6, 12]
    res = wide.resample_wide(pool, tr, nv, 0, R, seed=11)
    E, _H = expected.expected_majority_exact(pool, tr, nv)              # [P][B] fractions
    bound = 5 * 0.5 / np.sqrt(P * R)
    assert abs(bound - 0.0161) < 1e-4
    for b in range(4):
        mean = float(sum(E[p][b] for p in range(P)) / P)
        dev = abs(res.accuracy(b) - mean)
        print(f"k={nv[b]} mirror={res.accuracy(b):.6f} exact={mean:.6f} deviation={dev:.4f} bound={bound:.4f}")
        assert dev <= bound


def test_wide_majority_records_through_a_mirror_engine():
    class MirrorEngine:
        def resample_wide(self, pool, truth, n_valid, resamples, seed, tokens=None, r_begin=0, p_offset=0, M=None):
            return wide.resample_wide(pool, truth, n_valid, r_begin, r_begin + resamples, seed, tokens=tokens, p_offset=p_offset, M=M or None)

    pool, tok, tr = pool_of(4, 600, 2025, 1)
    limits = [2 ** 11, 2 ** 12, 300 * 2 ** 11, 600 * 2 ** 11]
    recs = curves.wide_majority_records(MirrorEngine(), pool, tr, tok, limits, 9, 17)
    res = wide.resample_wide(pool, tr, [1, 2, 300, 600], 0, 9, seed=17, tokens=tok)
    assert [set(r) for r in recs] == [{"token_limit", "accuracy", "avg_tokens_used"}] * 4
    assert [r["token_limit"] for r in recs] == limits
    assert [r["accuracy"] for r in recs] == [res.accuracy(b) for b in range(4)]
    assert [r["avg_tokens_used"] for r in recs] == [float(res.avg_tokens_used(b)) for b in range(4)]
    with pytest.raises(ValueError):
        curves.wide_majority_records(MirrorEngine(), pool, tr, tok, [601 * 2 ** 11], 9, 17)
