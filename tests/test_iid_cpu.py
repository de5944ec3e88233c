"""CPU tests of the vote over draws with replacement (include/scvote.h: scv_iid_prefix_i32): the numpy mirror
(o1_inference_scaling_laws_amd/iid.py) against a naive loop written from the header text (tests/independent_iid.py), the streams of
different resamples, the exact expectation by enumeration, and the k -> infinity record of the curve helper."""
import itertools
import statistics
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import curves, iid
from tests import independent_iid as naive


def small_case(k):
    """~200 small pools: N = 1 ... 9, budgets in -2 ... 20, ragged, duplicated and negative, tokens present and absent."""
    rng = np.random.default_rng(1000 + k)
    N = 1 + k % 9
    P = 1 + k % 3
    R = 1 + (k // 3) % 4
    B = (1, 3, 8, 32)[k % 4]
    values = (2, 3, 5, 1024)[(k // 2) % 4]                            # few values: ties; 1024: one past the bins now and then
    pool = rng.integers(0, values, size=(P, N)).astype(np.int32)
    if k % 7 == 0:
        pool[0, 0] = -5                                               # out of domain: bin 1023, error bit 0
    truth = np.where(rng.random(P) < 0.7, pool[:, 0], rng.integers(0, values + 1, size=P)).astype(np.int32)
    if k % 11 == 0:
        truth[0] = 1023                                               # meets the clamped votes
    if k % 13 == 0:
        truth[-1] = 5000                                              # outside the bins: never hits
    nd = rng.integers(-2, 21, size=B).astype(np.int32)
    nd[0] = (0, 1, 20, N)[k % 4]
    tokens = rng.integers(0, 3000, size=(P, N)).astype(np.int32) if k % 2 else None
    r0 = (0, 5, 2 ** 31 - 1 - R)[k % 3]
    p_off = (0, 2 ** 33)[(k // 5) % 2]
    M = (0, 1, 2, N + 1)[(k // 4) % 4]
    return pool, truth, nd, r0, R, 77 + k, tokens, p_off, M


@pytest.mark.parametrize("block", range(8))
def test_mirror_equals_the_naive_loop(block):
    for k in range(25 * block, 25 * block + 25):
        pool, truth, nd, r0, R, seed, tokens, p_off, M = small_case(k)
        got = iid.iid_prefix(pool, truth, nd, r0, r0 + R, seed, tokens=tokens, p_offset=p_off, M=M)
        tie, tsum, tcsum, per, err = naive.iid_prefix(pool.tolist(), truth.tolist(), nd.tolist(), r0, r0 + R, seed,
                                                      tokens=None if tokens is None else tokens.tolist(), p_offset=p_off, M=M)
        assert got.tie_class_hits.tolist() == tie, k
        assert got.truth_count_sum.tolist() == tcsum, k
        assert got.token_sum.tolist() == tsum, k
        assert (got.per_resample is None) == (per is None), k
        if per is not None:
            assert got.per_resample.tolist() == per, k
        assert got.error_bits == err, k
        assert (got.P, got.R) == (pool.shape[0], R)


def test_mirror_draws_are_the_header_formula():
    s = int(iid.problem_streams(9, np.array([4 + 2 ** 33]))[0])
    assert s == naive.mix64((9 ^ 0xA0761D6478BD642F) + naive.G * (4 + 2 ** 33 + 1))
    for r, i, N in ((0, 0, 1), (3, 17, 7), (2 ** 31 - 2, 65534, 256)):
        u = naive.mix64(s + naive.G * (r * 65536 + i + 1))
        assert int(iid.draw_index(np.uint64(s), np.uint64(r), i, N)) == ((u >> 32) * N) >> 32


def test_a_budget_above_the_limit_computes_nothing():
    pool = np.array([[1, 1, 2]], dtype=np.int32)
    got = iid.iid_prefix(pool, np.array([1]), np.array([3, iid.MAX_DRAWS + 1]), 0, 4, 1, M=2)
    assert got.error_bits == iid.ERR_DRAWS_BIT and not got.tie_class_hits.any() and not got.per_resample.any()
    ok = iid.iid_prefix(pool, np.array([1]), np.array([3]), 0, 4, 1)
    assert ok.error_bits == 0 and ok.tie_class_hits.sum() > 0


def test_streams_of_different_resamples_do_not_overlap():
    """The counters r * 65536 + i + 1, i < 65535, of different r are distinct: resample r owns (r * 65536, r * 65536 + 65535]."""
    assert iid.R_STRIDE == 65536 and iid.MAX_DRAWS == 65535 and iid.MAX_DRAWS < iid.R_STRIDE
    rng = np.random.default_rng(5)
    rs = np.unique(np.concatenate([np.array([0, 1, 2, 2 ** 31 - 2, 2 ** 31 - 1]), rng.integers(0, 2 ** 31, size=300)]))
    first = np.array([naive.draw_counter(int(r), 0) for r in rs], dtype=object)
    last = np.array([naive.draw_counter(int(r), 65534) for r in rs], dtype=object)
    assert all(lo <= hi for lo, hi in zip(first, last))
    assert all(last[j] < first[j + 1] for j in range(len(rs) - 1))              # rs ascending: the ranges are disjoint intervals
    assert last[-1] < 2 ** 64                                                    # ... and no counter wraps
    sample = set()
    n = 0
    for r in (0, 1, 7, 2 ** 31 - 1):
        for i in (0, 1, 2, 1000, 65533, 65534):
            sample.add(naive.draw_counter(r, i))
            n += 1
    assert len(sample) == n


def exact_score(row, truth, k):
    total = Fraction(0)
    for seq in itertools.product(row, repeat=k):
        modes = statistics.multimode(seq)
        if truth in modes:
            total += Fraction(1, len(modes))
    return total / len(row) ** k


@pytest.mark.parametrize("row,truth", [((4, 4, 9), 4), ((4, 4, 9), 9), ((4, 9, 2), 9)])
def test_mean_over_resamples_meets_the_exact_enumeration(row, truth):
    """All N^k draw sequences give the exact expected score; with R = 40 000 the mirror's mean lies within 4 * 0.5 / sqrt(R) = 0.01 of it
    (a score lies in [0, 1]: standard deviation <= 0.5).  Fixed seeds."""
    R = 40_000
    ks = [1, 2, 3, 4, 5]
    pool = np.array([row], dtype=np.int32)
    for seed in (1, 2024):
        got = iid.iid_prefix(pool, np.array([truth]), np.array(ks), 0, R, seed)
        for b, k in enumerate(ks):
            want = float(exact_score(row, truth, k))
            print(row, truth, seed, k, got.accuracy(b), want)
            assert abs(got.accuracy(b) - want) <= 4 * 0.5 / np.sqrt(R), (seed, k)


class FakeEngine:
    """The two Engine methods iid_majority_records calls, on the CPU."""

    def iid_prefix(self, pool, truth, n_draws, resamples, seed, tokens=None, r_begin=0, p_offset=0, M=None):
        return iid.iid_prefix(pool, truth, n_draws, r_begin, r_begin + resamples, seed, tokens=tokens, p_offset=p_offset, M=M or 0)

    def aggregate_prefix(self, pool, truth, n_valid, tokens=None, want_cells=True):
        score = []
        for row, t in zip(np.asarray(pool).tolist(), np.asarray(truth).tolist()):
            modes = statistics.multimode(row[: int(n_valid[0])])
            score.append(1.0 / len(modes) if t in modes else 0.0)

        class Whole:
            def accuracy(self, b=0):
                return float(np.mean(score))
        return Whole()


def test_the_last_record_is_the_vote_over_the_whole_pool():
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 4, size=(12, 9)).astype(np.int32)
    truth = pool[:, 0].copy()
    tokens = rng.integers(1, 2048, size=pool.shape).astype(np.int32)
    draws = [1, 4, 9, 30, 200]
    recs = curves.iid_majority_records(FakeEngine(), pool, truth, tokens, draws, 50, 7)
    assert [r["samples"] for r in recs[:-1]] == draws and recs[-1]["samples"] == float("inf")
    whole = np.mean([1.0 / len(statistics.multimode(r)) if t in statistics.multimode(r) else 0.0 for r, t in zip(pool.tolist(), truth.tolist())])
    assert recs[-1] == {"samples": float("inf"), "accuracy": float(whole)}
    res = iid.iid_prefix(pool, truth, np.array(draws), 0, 50, 7, tokens=tokens)
    assert [r["accuracy"] for r in recs[:-1]] == [res.accuracy(b) for b in range(5)]
    assert [r["avg_tokens_used"] for r in recs[:-1]] == [float(res.avg_tokens_used(b)) for b in range(5)]
    # the reference's grid, past the pool: T // 2^11 draws, no refusal
    limits = [2 ** 11, 2 ** 13, 2 ** 16]
    grid = curves.iid_majority_records(FakeEngine(), pool, truth, None, None, 20, 7, token_limits=limits)
    assert [r["samples"] for r in grid] == [1, 4, 32, float("inf")] and [r["token_limit"] for r in grid[:-1]] == limits
    assert all(r["avg_tokens_used"] == 0.0 for r in grid[:-1])
    with pytest.raises(ValueError):
        curves.iid_majority_records(FakeEngine(), pool, truth, None, None, 20, 7, token_limits=[1024])
