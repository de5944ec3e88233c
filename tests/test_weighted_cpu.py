"""CPU tests of the weighted majority vote / best-of-N (scv_weighted_prefix_i32): the numpy mirror (o1_inference_scaling_laws_amd/weighted.py)
against an independent pure-Python restatement of the header text (tests/independent_weighted.py), its reduction to the plain-vote mirrors
under unit weights, invariance under scaling of the weights, quantize_weights, the error bits and the argument errors.  No GPU needed."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import resample, synth, token_budget, weighted
from o1_inference_scaling_laws_amd.scoring import exact_accuracy_from_tie_classes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import independent_weighted as ind  # noqa: E402

WMAX = weighted.WEIGHT_MAX


def pool_of(P, N, seed, dist=1):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    return a[:, 0, :].copy(), t[:, 0, :].copy(), tr


def weights_for(pool, seed):
    """Small weights (many ties), zeros, WEIGHT_MAX; row 0 all equal, row 1 all zero, row 2 all WEIGHT_MAX."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, size=pool.shape)
    big = rng.random(pool.shape) < 0.2
    w[big] = rng.integers(0, WMAX + 1, size=int(big.sum()))
    w[rng.random(pool.shape) < 0.05] = WMAX
    for row, val in ((0, 7), (1, 0), (2, WMAX)):
        if row < pool.shape[0]:
            w[row] = val
    return w.astype(np.int32)


@pytest.mark.parametrize("N", [1, 2, 3, 8, 63, 64, 65, 128, 255, 256])
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("shuffled", [False, True])
def test_mirror_against_the_independent_restatement(N, rule, shuffled):
    P = 4
    pool, tok, tr = pool_of(P, N, 100 + N, dist=(1, 3, 0)[N % 3])
    tr[3] = 2000 if N % 2 else tr[3]                                     # a truth outside the bins never hits
    w = weights_for(pool, N)
    rng = np.random.default_rng(N)
    nv = np.array([0, 1, N, N + 5, -2] + rng.integers(0, N + 1, size=3).tolist(), dtype=np.int32)
    r0, r1 = (5, 8) if shuffled else (0, None)
    got = weighted.weighted_prefix(pool, w, tr, nv, rule, r0, r1, seed=11, p_offset=2 ** 33 + 1, M=N + 1, tokens=tok, want_cells=not shuffled)
    tie, score, toks, cells = ind.weighted_prefix(pool.tolist(), w.tolist(), tr.tolist(), nv.tolist(), rule, r0, r1, 11, 2 ** 33 + 1,
                                                  tokens=tok.tolist())
    assert got.error_bits == 0
    R = 3 if shuffled else 1
    for b in range(len(nv)):
        assert {m: int(c) for m, c in enumerate(got.tie_class_hits[b]) if c} == tie[b]
        assert exact_accuracy_from_tie_classes(got.tie_class_hits[b], P * R) == score[b] / (P * R)
        assert int(got.token_sum[b]) == toks[b]
        assert np.array_equal(got.per_resample[:, b, :].sum(axis=0), got.tie_class_hits[b, :N + 1])
    if not shuffled:
        for p in range(P):
            for b in range(len(nv)):
                c = got.cells[p, b]
                assert (int(c["max_count"]), int(c["truth_count"]), int(c["n_modes"]), int(c["min_mode"]), int(c["hit"])) == cells[p][b]


def test_the_shuffle_of_the_restatement_is_the_mirrors():
    perm = token_budget.orderings(2, 37, 4, 6, 9, p_offset=3)
    for p in range(2):
        for r in range(2):
            assert perm[p * 2 + r].tolist() == ind.permutation(9, 3 + p, 4 + r, 37)


@pytest.mark.parametrize("N", [1, 8, 65, 256])
def test_unit_weights_are_the_plain_vote(N):
    pool, tok, tr = pool_of(6, N, N)
    nv = np.array([0, 1, N // 2, N, N + 1], dtype=np.int32)
    ones = np.ones_like(pool)
    got = weighted.weighted_prefix(pool, ones, tr, nv, 0, 3, 9, seed=5, p_offset=7, M=N + 1, tokens=tok)
    want = resample.resample_prefix(pool, tr, nv, 3, 9, 5, tokens=tok, p_offset=7, M=N + 1)
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
    assert np.array_equal(got.token_sum, want.token_sum)
    # token budgets with every sample at one token are sample counts
    tb = token_budget.token_budget_prefix(pool, ones, tr, np.clip(nv, 0, None).astype(np.int64), 3, 9, 5, 7, M=N + 1)
    assert np.array_equal(got.tie_class_hits, tb.tie_class_hits) and np.array_equal(got.per_resample, tb.per_resample)
    po = weighted.weighted_prefix(pool, ones, tr, nv, 0, want_cells=True)
    tp = token_budget.token_budget_prefix(pool, ones, tr, np.clip(nv, 0, None).astype(np.int64), want_cells=True)
    assert np.array_equal(po.tie_class_hits, tp.tie_class_hits) and np.array_equal(po.cells, tp.cells)


@pytest.mark.parametrize("rule", [0, 1])
def test_scaling_every_weight_changes_no_tie_table(rule):
    pool, _, tr = pool_of(8, 40, 3)
    w = np.random.default_rng(1).integers(0, 1000, size=pool.shape).astype(np.int32)
    nv = np.array([1, 5, 17, 40], dtype=np.int32)
    a = weighted.weighted_prefix(pool, w, tr, nv, rule, 0, 6, 2, M=41)
    b = weighted.weighted_prefix(pool, w * (WMAX // 999), tr, nv, rule, 0, 6, 2, M=41)
    assert np.array_equal(a.tie_class_hits, b.tie_class_hits) and np.array_equal(a.per_resample, b.per_resample)
    assert int((w * (WMAX // 999)).max()) <= WMAX


def test_best_of_ties_between_votes():
    """Rule 1: two samples of different votes tie for the top weight -> a tie between those votes; a higher weight breaks it."""
    pool = np.array([[4, 9, 4, 2]], dtype=np.int32)
    w = np.array([[5, 5, 1, 3]], dtype=np.int32)
    nv = np.array([1, 2, 4], dtype=np.int32)
    got = weighted.weighted_prefix(pool, w, np.array([9]), nv, 1, want_cells=True)
    assert [int(got.tie_class_hits[b].argmax()) if got.tie_class_hits[b].any() else 0 for b in range(3)] == [0, 2, 2]
    assert got.exact_accuracy(1) == Fraction(1, 2)
    assert got.cells["min_mode"].tolist() == [[4, 4, 4]] and got.cells["max_count"].tolist() == [[5, 5, 5]]
    s = weighted.weighted_prefix(pool, w, np.array([9]), nv, 0, want_cells=True)          # rule 0: value 4 sums to 6 and wins alone
    assert s.cells["max_count"].tolist() == [[5, 5, 6]] and s.cells["n_modes"].tolist() == [[1, 2, 1]] and not s.cells["hit"][0, 2]


def test_quantize_weights():
    rng = np.random.default_rng(0)
    s = np.sort(rng.normal(size=5000))
    w = weighted.quantize_weights(s)
    assert w.dtype == np.int32 and w[0] == 0 and w[-1] == WMAX and (np.diff(w.astype(np.int64)) >= 0).all()
    w = weighted.quantize_weights(s, lo=-1.0, hi=1.0)
    assert w.min() == 0 and w.max() == WMAX and (np.diff(w.astype(np.int64)) >= 0).all()
    assert weighted.quantize_weights([0.0, 0.5, 1.0]).tolist() == [0, (WMAX + 1) // 2, WMAX]          # round half up: 8388607.5 -> 8388608
    assert weighted.quantize_weights([3.0, 3.0]).tolist() == [WMAX, WMAX]
    assert weighted.quantize_weights(np.zeros((2, 0))).shape == (2, 0)
    with pytest.raises(ValueError):
        weighted.quantize_weights([1.0, float("nan")])
    with pytest.raises(ValueError):
        weighted.quantize_weights([1.0], lo=2.0, hi=1.0)


def test_error_bits():
    pool, _, tr = pool_of(3, 8, 1)
    w = np.ones_like(pool)
    nv = np.array([8], dtype=np.int32)
    assert weighted.weighted_prefix(pool, w, tr, nv).error_bits == 0
    for bad in (-1, WMAX + 1):
        wb = w.copy()
        wb[2, 7] = bad
        assert weighted.weighted_prefix(pool, wb, tr, nv).error_bits == weighted.ERR_WEIGHT_BIT == 32
    pb = pool.copy()
    pb[0, 0] = 1024
    assert weighted.weighted_prefix(pb, w, tr, nv).error_bits == resample.ERR_DOMAIN_BIT == 1
    tie8 = np.tile(np.arange(8, dtype=np.int32), (3, 1))
    r = weighted.weighted_prefix(tie8, w, np.array([0, 1, 2]), nv, 1, 0, 2, 1, M=8)
    assert r.error_bits == resample.ERR_CLASS_BIT == 2 and r.tie_class_hits[0, 8] == 6 and not r.per_resample.any()
    assert weighted.weighted_prefix(tie8, w, np.array([0, 1, 2]), nv, 1, 0, 2, 1, M=9).error_bits == 0


def test_argument_errors_raise():
    pool, tok, tr = pool_of(2, 8, 1)
    w = np.ones_like(pool)
    nv = np.array([8], dtype=np.int32)
    for kw in (dict(rule=2), dict(r_begin=1), dict(r_begin=3, r_end=2), dict(M=0), dict(r_end=2, want_cells=True), dict(p_offset=-1),
               dict(tokens=tok[:, :4])):
        with pytest.raises(ValueError):
            weighted.weighted_prefix(pool, w, tr, nv, **kw)
    for args in ((pool, None, tr, nv), (pool, w[:, :4], tr, nv), (pool, w, tr[:1], nv), (pool[0], w[0], tr, nv),
                 (pool, w, tr, np.ones(33, dtype=np.int32)), (np.zeros((2, 257), dtype=np.int32), np.ones((2, 257), dtype=np.int32), tr, nv)):
        with pytest.raises(ValueError):
            weighted.weighted_prefix(*args)
