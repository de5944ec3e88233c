"""CPU tests of short-m@k (scv_shortest_prefix_i32, include/scvote.h): the numpy mirror (o1_inference_scaling_laws_amd/shortest.py) against a
naive per-ordering loop written from the header text (tests/independent_shortest.py), the three identities of the header against the mirror of
scv_resample_prefix_i32 (resample.py), and the exact enumeration of all orderings of small pools against the mean over them."""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import resample, shortest, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import independent_shortest as ind  # noqa: E402


def pool_of(P, N, seed, dist=1, tok_values=None):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    pool, tok = a[:, 0, :].copy(), t[:, 0, :].copy()
    if tok_values is not None:                                          # few distinct token counts: the pool-index tie-break decides
        tok = np.random.default_rng(seed).choice(np.asarray(tok_values, dtype=np.int32), size=pool.shape).astype(np.int32)
    return pool, tok, tr


def pairs_for(N, B, seed):
    """ragged, unsorted, duplicated: k = 0, k > N, m = 0, m < 0, m > k."""
    rng = np.random.default_rng(seed)
    base = [(0, 0), (0, 3), (N + 5, 1), (N, N), (N, 0), (N, -2), (1, 1), (max(N // 2, 1), N + 3), (N, max(N // 4, 1))]
    base += [(int(k), int(rng.integers(-1, k + 2))) for k in rng.integers(0, N + 1, size=8)]
    pick = rng.integers(0, len(base), size=B)
    return np.array([base[i][0] for i in pick], dtype=np.int32), np.array([base[i][1] for i in pick], dtype=np.int32)


def assert_matches_independent(got, want, P, B, cells):
    assert np.array_equal(got.tie_class_hits, want["tie"])
    assert np.array_equal(got.voted_token_sum, want["voted"]) and np.array_equal(got.spent_token_sum, want["spent"])
    assert np.array_equal(got.latency_sum, want["latency"]) and np.array_equal(got.truth_count_sum, want["truth_sum"])
    assert np.array_equal(got.per_resample, want["per"])
    if cells:
        for p in range(P):
            for b in range(B):
                c = got.cells[p, b]
                assert (int(c["max_count"]), int(c["truth_count"]), int(c["n_modes"]), int(c["min_mode"]), int(c["hit"]),
                        int(got.cell_tokens[p, b])) == want["cells"][(p, b)], (p, b)


@pytest.mark.parametrize("N", [1, 2, 5, 31, 32, 33, 64, 65])
@pytest.mark.parametrize("shuffled", [False, True])
def test_mirror_matches_the_naive_loop(N, shuffled):
    for draw in range(3):
        k = 7 * N + draw
        P, B, R = 2 + k % 3, (1, 5, 32)[k % 3], (1, 3, 9)[k % 3]
        pool, tok, tr = pool_of(P, N, 100 + k, dist=draw % 6, tok_values=(None, (7, 9), (0, 0, 5))[draw])
        tr[0] = 1022                                                    # (mostly) a truth absent from the row
        nv, mk = pairs_for(N, B, k)
        r0, p_off = (0, 11)[k % 2], (0, 1 << 33)[draw % 2]
        M = N + 1
        got = shortest.shortest_prefix(pool, tok, tr, nv, mk, r0 if shuffled else 0, r0 + R if shuffled else None, seed=5 + k,
                                       p_offset=p_off, M=M, want_cells=not shuffled)
        assert got.error_bits == 0
        want = ind.shortest(pool, tok, tr, nv, mk, r0, r0 + R if shuffled else None, 5 + k, p_off, M)
        assert_matches_independent(got, want, P, B, cells=not shuffled)


def test_open_domain_mirror_matches_the_naive_loop():
    rng = np.random.default_rng(3)
    vals = np.array([-2 ** 31, -7, 0, 1023, 1024, 2 ** 31 - 1, 123456789], dtype=np.int64)
    pool = rng.choice(vals, size=(4, 20)).astype(np.int32)
    tok = rng.integers(0, 50, size=pool.shape).astype(np.int32)
    tr = np.array([-7, 2 ** 31 - 1, 5, -2 ** 31], dtype=np.int32)
    nv, mk = pairs_for(20, 6, 3)
    got = shortest.shortest_prefix(pool, tok, tr, nv, mk, 0, 4, seed=1, M=21, open_domain=True)
    want = ind.shortest(pool, tok, tr, nv, mk, 0, 4, 1, 0, 21, open_domain=True)
    assert got.error_bits == 0
    assert_matches_independent(got, want, 4, 6, cells=False)
    cells = shortest.shortest_prefix(pool, tok, tr, nv, mk, want_cells=True, open_domain=True)
    ref = ind.shortest(pool, tok, tr, nv, mk, 0, None, 0, 0, 21, open_domain=True)
    for (p, b), c in ref["cells"].items():                              # min_mode is the CODE: the rank of the value in its row
        code = -1 if c[3] == -1 else int(np.searchsorted(np.unique(pool[p]), c[3]))
        assert int(cells.cells[p, b]["min_mode"]) == code and int(cells.cells[p, b]["max_count"]) == c[0]


@pytest.mark.parametrize("N", [1, 8, 33, 128])
def test_keeping_every_sample_is_the_resampled_vote(N):
    """m_b >= k_b: tie classes, truth counts and per_resample of resample.py bit for bit, voted = spent = its token sum, and the latency is the
    largest token count of the prefix."""
    pool, tok, tr = pool_of(5, N, N, dist=1)
    rng = np.random.default_rng(N)
    nv = np.concatenate([[0, 1, N, N + 3], rng.integers(0, N + 1, size=4)]).astype(np.int32)
    mk = nv + rng.integers(0, 3, size=nv.shape).astype(np.int32)
    got = shortest.shortest_prefix(pool, tok, tr, nv, mk, 2, 12, seed=9, p_offset=3, M=N + 1)
    want = resample.resample_prefix(pool, tr, nv, 2, 12, 9, tokens=tok, p_offset=3, M=N + 1)
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
    assert np.array_equal(got.truth_count_sum, want.truth_count_sum)
    assert np.array_equal(got.voted_token_sum, want.token_sum) and np.array_equal(got.spent_token_sum, want.token_sum)
    from o1_inference_scaling_laws_amd.token_budget import orderings
    perm = orderings(5, N, 2, 12, 9, 3).reshape(5, 10, N)
    for b, k in enumerate(np.clip(nv, 0, N)):
        lat = sum(int(tok[p, perm[p, r, :k]].max()) for p in range(5) for r in range(10)) if k else 0
        assert int(got.latency_sum[b]) == lat


def test_the_whole_pool_does_not_depend_on_the_ordering():
    """k_b = N: S is the whole pool whatever the ordering, so every ordering gives the same cell."""
    N = 40
    pool, tok, tr = pool_of(4, N, 8, dist=3, tok_values=(3, 4, 5))
    nv = np.full(6, N, dtype=np.int32)
    mk = np.array([1, 2, 7, 20, 39, 40], dtype=np.int32)
    one = shortest.shortest_prefix(pool, tok, tr, nv, mk, want_cells=True)
    for seed, r0, R in ((1, 0, 5), (2, 100, 3)):
        many = shortest.shortest_prefix(pool, tok, tr, nv, mk, r0, r0 + R, seed=seed, M=N + 1)
        assert np.array_equal(many.tie_class_hits, R * one.tie_class_hits)
        assert np.array_equal(many.spent_token_sum, R * one.spent_token_sum) and np.array_equal(many.latency_sum, R * one.latency_sum)
        assert np.array_equal(many.voted_token_sum, R * one.voted_token_sum) and np.array_equal(many.truth_count_sum, R * one.truth_count_sum)
        assert (many.per_resample == many.per_resample[0]).all()


def test_equal_tokens_keep_the_lowest_pool_indices():
    """All tokens equal: V is the m_b lowest pool indices of S.  In pool order that is the prefix of m_b samples: the vote of
    resample.py's machinery over n_valid = m_b in the identity order -- checked here against a direct count."""
    N, t = 30, 17
    pool, _, tr = pool_of(6, N, 4, dist=1)
    tok = np.full_like(pool, t)
    nv = np.array([30, 20, 10, 5, 30], dtype=np.int32)
    mk = np.array([4, 20, 3, 9, 30], dtype=np.int32)
    got = shortest.shortest_prefix(pool, tok, tr, nv, mk, want_cells=True)
    for b, (k, m) in enumerate(zip(nv, np.minimum(mk, nv))):
        for p in range(6):
            vals, counts = np.unique(pool[p, :m], return_counts=True)
            c = got.cells[p, b]
            assert int(c["max_count"]) == counts.max() and int(c["n_modes"]) == (counts == counts.max()).sum()
            assert int(c["min_mode"]) == vals[counts.argmax()]
            assert int(got.cell_tokens[p, b]) == k * t
    assert np.array_equal(got.latency_sum, np.full(5, 6 * t)) and np.array_equal(got.voted_token_sum, 6 * t * np.minimum(mk, nv))
    # shuffled: the kept samples are the m lowest pool indices among the first k of the ordering
    from o1_inference_scaling_laws_amd.token_budget import orderings
    sh = shortest.shortest_prefix(pool, tok, tr, nv, mk, 0, 3, seed=6, M=N + 1)
    perm = orderings(6, N, 0, 3, 6).reshape(6, 3, N)
    for b, (k, m) in enumerate(zip(nv, np.minimum(mk, nv))):
        tc = sum(int((pool[p, np.sort(perm[p, r, :k])[:m]] == tr[p]).sum()) for p in range(6) for r in range(3))
        assert int(sh.truth_count_sum[b]) == tc


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
def test_all_orderings_enumerated(N):
    """The exact expectation of short-m@k over ALL N! orderings of a small pool, as a rational, against the kernel's estimator run over each of
    them once (the mean over orderings is what the shuffled call estimates; here every ordering is fed as its own pool in pool order)."""
    rng = np.random.default_rng(N)
    votes = rng.integers(0, 3, size=N).astype(np.int32)
    toks = rng.integers(1, 4, size=N).astype(np.int32)                  # ties in the tokens: the pool index decides
    truth = int(votes[0])
    perms = list(itertools.permutations(range(N)))
    pairs = [(k, m) for k in range(N + 1) for m in range(k + 1)]
    # exact, from the definition: V depends on the SET of the first k samples only
    exact = {}
    for k, m in pairs:
        acc = Fraction(0)
        for pi in perms:
            V = ind.kept(list(pi), toks.tolist(), k, m)
            vv = [int(votes[x]) for x in V]
            if vv:
                cnt = {v: vv.count(v) for v in vv}
                top = max(cnt.values())
                modes = [v for v, c in cnt.items() if c == top]
                if truth in modes:
                    acc += Fraction(1, len(modes))
        exact[(k, m)] = acc / len(perms)
    # the mirror must see the ORIGINAL pool indices for its tie-break: run the pool order on each permuted pool with the index folded into the
    # token key (tokens * N + original index keeps the order of (tokens, index) pairs and has no ties)
    pool = np.array([[votes[x] for x in pi] for pi in perms], dtype=np.int32)
    tok = np.array([[int(toks[x]) * N + x for x in pi] for pi in perms], dtype=np.int32)
    tr = np.full(len(perms), truth, dtype=np.int32)
    for i in range(0, len(pairs), 32):
        part = pairs[i:i + 32]
        res = shortest.shortest_prefix(pool, tok, tr, [k for k, _ in part], [m for _, m in part])
        for b, km in enumerate(part):
            assert res.exact_accuracy(b) == exact[km], km


def test_argument_checks_and_error_bits():
    pool, tok, tr = pool_of(2, 8, 1)
    nv, mk = np.array([4, 8], dtype=np.int32), np.array([2, 8], dtype=np.int32)
    with pytest.raises(ValueError):
        shortest.shortest_prefix(pool, tok, tr, nv, mk[:1])
    with pytest.raises(ValueError):
        shortest.shortest_prefix(pool, tok, tr, nv, mk, 1, None)
    with pytest.raises(ValueError):
        shortest.shortest_prefix(pool, tok, tr, nv, mk, 0, 3, want_cells=True)
    with pytest.raises(ValueError):
        shortest.shortest_prefix(np.zeros((1, 257), np.int32), np.zeros((1, 257), np.int32), tr[:1], nv, mk)
    bad_tok = tok.copy()
    bad_tok[1, 7] = -1
    assert shortest.shortest_prefix(pool, bad_tok, tr, nv, mk).error_bits == 16
    bad_pool = pool.copy()
    bad_pool[0, 0] = 5000
    assert shortest.shortest_prefix(pool * 0 + bad_pool, tok, tr, nv, mk).error_bits == 1
    flat = np.tile(np.arange(8, dtype=np.int32), (2, 1))                # an 8-way tie at m = 8
    assert shortest.shortest_prefix(flat, tok, np.array([0, 1], np.int32), nv, mk, 0, 2, M=8).error_bits == 2
    empty = shortest.shortest_prefix(pool[:0], tok[:0], tr[:0], nv, mk, 0, 3, M=4)
    assert not empty.tie_class_hits.any() and empty.per_resample.shape == (3, 2, 4)
