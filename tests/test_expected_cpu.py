"""CPU tests of the exact expected majority vote (o1_inference_scaling_laws_amd/expected.py, the statement of scv_expected_majority_i32):
the rational form against brute-force enumeration with statistics.multimode, the k = 1, 2, N identities, the exactness of the
Gauss-Legendre form (the GPU's algorithm) up to N = 256, the ABI declaration and binding, and the schema of
curves.exact_majority_records."""
import itertools
import math
import os
import re
import statistics
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import curves, expected

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(row, truth, k, clamp=True):
    """Mean over all k-subsets of the reference's score (o1.py:202-213) and of the hit indicator."""
    v = [x if 0 <= x < 1024 else 1023 for x in row] if clamp else list(row)
    if k == 0:
        return Fraction(0), Fraction(0)
    e, h, n = Fraction(0), Fraction(0), 0
    for sub in itertools.combinations(range(len(v)), k):
        modes = statistics.multimode([v[i] for i in sub])
        n += 1
        if 0 <= truth < 1024 and truth in modes:
            e += Fraction(1, len(modes))
            h += 1
    return e / n, h / n


def by_chunks(fn, row, truth, ks):
    """fn over budgets in calls of at most 32 (the limit of B): two lists over ks."""
    a, b = [], []
    for i in range(0, len(ks), 32):
        x, y = fn([row], [truth], ks[i:i + 32])
        a += list(x[0])
        b += list(y[0])
    return a, b


def random_pools(seed, count, nmax=14):
    rng = np.random.default_rng(seed)
    for i in range(count):
        N = int(rng.integers(1, nmax + 1))
        V = int(rng.integers(1, 6))
        row = rng.integers(0, V, size=N).tolist()
        truth = int(rng.integers(0, V + 1))                         # V: the truth is absent
        if i % 6 == 0:
            truth = 1500                                               # outside the bins: never hits
        if i % 5 == 0:
            row[int(rng.integers(0, N))] = int(rng.choice([-3, 1024, 5000]))   # outside the domain: counts as 1023
            if i % 10 == 0:
                truth = 1023                                           # ... and can hit as 1023
        yield row, truth


def test_rationals_match_brute_force_for_every_k():
    for row, truth in random_pools(1, 70):
        N = len(row)
        ks = list(range(N + 1))
        E, H = expected.expected_majority_exact([row], [truth], ks)
        for k in ks:
            be, bh = brute(row, truth, k)
            assert E[0][k] == be and H[0][k] == bh, (row, truth, k)


def test_ties_everywhere():
    row = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]                        # every class ties at every j
    for truth in (0, 5, 9):
        E, H = expected.expected_majority_exact([row], [truth], list(range(13)))
        for k in range(13):
            assert (E[0][k], H[0][k]) == brute(row, truth, k)


def test_domain_flag_and_clamp_semantics():
    row = [3, -1, 1023, 3, 2000]
    assert expected.domain_error([row]) and not expected.domain_error([[3, 1023]])
    E, H = expected.expected_majority_exact([row], [1023], [1, 2, 3, 5])
    assert [E[0][i] for i in range(4)] == [brute(row, 1023, k)[0] for k in (1, 2, 3, 5)]
    assert E[0][0] == Fraction(3, 5)                                   # three votes count as 1023


def test_identities_k1_k2_kN():
    rng = np.random.default_rng(3)
    for _ in range(40):
        N = int(rng.integers(2, 60))
        row = rng.integers(0, int(rng.integers(1, 8)), size=N).tolist()
        truth = row[0] if rng.random() < 0.8 else 77
        ct = row.count(truth)
        E, H = expected.expected_majority_exact([row], [truth], [1, 2, N])
        assert E[0][0] == E[0][1] == Fraction(ct, N) and H[0][0] == Fraction(ct, N)
        modes = statistics.multimode(row)
        assert E[0][2] == (Fraction(1, len(modes)) if truth in modes else 0)


def test_no_tie_closed_form_and_j1_recurrence():
    # c_t = 30 against at most 3 votes of any other value: terms with j > 3 truth votes come from the closed form C(c_t, j) C(N - c_t, k - j)
    row = [7] * 30 + [1, 2, 2, 3, 3, 3]
    E, H = by_chunks(expected.expected_majority_exact, row, 7, list(range(37)))
    for k in list(range(5)) + list(range(33, 37)):
        assert (E[k], H[k]) == brute(row, 7, k)
    for k in range(5, 33):                                             # ties only cost score: the hit probability bounds it from above
        assert H[k] >= E[k] > 0
    # j = 1 only: every other value once -> E_k = c_t e_{k-1}(1, ..., 1) / (k C(N, k))
    row = [0] + list(range(1, 10))
    E, _ = expected.expected_majority_exact([row], [0], list(range(1, 11)))
    for k in range(1, 11):
        assert E[0][k - 1] == Fraction(math.comb(9, k - 1), k * math.comb(10, k))


def _max_u_pools():
    """Pools that maximise U_j: c_t = j and as many other classes of exactly j votes as fit, up to N = 256."""
    out = []
    for N, j in ((256, 2), (256, 3), (255, 4), (200, 2), (129, 8), (128, 2), (64, 16), (256, 128), (256, 1)):
        row = [0] * j + sum([[v] * j for v in range(1, (N - j) // j + 1)], [])
        row += [999] * (N - len(row))
        out.append((row, 0))
    return out


@pytest.mark.parametrize("idx", range(9))
def test_quadrature_within_1e12_of_the_rationals(idx):
    row, truth = _max_u_pools()[idx]
    N = len(row)
    ks = sorted({1, 2, 3, 4, 5, 8, 16, 17, 32, 64, 100, 128, 129, 200, 255, 256} & set(range(N + 1)))[:32]
    E, H = expected.expected_majority_exact([row], [truth], ks)
    s, h = expected.expected_majority_quadrature([row], [truth], ks)
    for b in range(len(ks)):
        for r, g in ((E[0][b], s[0, b]), (H[0][b], h[0, b])):
            if r == 0:
                assert g == 0.0
            else:
                assert abs(g - float(r)) <= 1e-12 * float(r), (ks[b], g, float(r))


def test_quadrature_on_random_pools():
    for row, truth in random_pools(9, 60, nmax=40):
        ks = list(range(len(row) + 1))
        E, H = by_chunks(expected.expected_majority_exact, row, truth, ks)
        s, h = by_chunks(expected.expected_majority_quadrature, row, truth, ks)
        for k in ks:
            for r, g in ((E[k], s[k]), (H[k], h[k])):
                assert (g == 0.0) if r == 0 else abs(g - float(r)) <= 1e-12 * float(r)


def test_header_and_binding_declare_the_symbol():
    hdr = open(os.path.join(REPO, "include", "scvote.h")).read()
    assert re.search(r"int scv_expected_majority_i32\(scv_ctx\* ctx, const int32_t\* pool, const int32_t\* n_valid, const int32_t\* truth,\s+"
                     r"int64_t P, int32_t B, int64_t N, int mem_kind,\s+double\* expected_score_out, double\* hit_prob_out\);", hdr)
    assert '"expected_calls"' in hdr
    lib = open(os.path.join(REPO, "o1_inference_scaling_laws_amd", "_lib.py")).read()
    assert "L.scv_expected_majority_i32.argtypes = [p, p, p, p, i64, i32, i64, C.c_int, p, p]" in lib
    src = open(os.path.join(REPO, "o1_inference_scaling_laws_amd", "csrc", "scvote.hip")).read()
    assert '"expected_calls"' in src and "int scv_expected_majority_i32(" in src


class _StubEngine:
    """The mirror in the place of the device (the CPU box has none)."""
    def expected_majority(self, pool, truth, n_valid, tokens=None, hit_prob=True):
        E, H = expected.expected_majority_exact(pool, truth, n_valid)
        N = np.asarray(pool).shape[1]
        return expected.ExpectedResult(np.array([[float(x) for x in r] for r in E]), None, np.clip(np.asarray(n_valid), 0, N), N,
                                       None if tokens is None else int(np.asarray(tokens, dtype=np.int64).sum()))


def test_exact_majority_records_schema():
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 4, size=(6, 8)).astype(np.int32)
    truth = pool[:, 0].copy()
    tokens = rng.integers(100, 2000, size=(6, 8)).astype(np.int32)
    limits = [2 ** 11, 2 ** 12, 2 ** 13, 2 ** 14]
    recs = curves.exact_majority_records(_StubEngine(), pool, truth, tokens, limits)
    assert [r["token_limit"] for r in recs] == limits
    assert all(set(r) == {"token_limit", "accuracy", "avg_tokens_used"} for r in recs)
    E, _ = expected.expected_majority_exact(pool, truth, [1, 2, 4, 8])
    for b, r in enumerate(recs):
        assert r["accuracy"] == math.fsum(float(E[p][b]) for p in range(6)) / 6
        assert r["avg_tokens_used"] == float(Fraction((1 << b) * int(tokens.astype(np.int64).sum()), 8 * 6))
    assert curves.exact_majority_records(_StubEngine(), pool, truth, None, limits)[0]["avg_tokens_used"] == 0.0
    with pytest.raises(ValueError):
        curves.exact_majority_records(_StubEngine(), pool, truth, None, [2 ** 15])
