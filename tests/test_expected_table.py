"""CPU proof of the table of scv_expected_majority_i32 (csrc/scvote_expected_table.h, plain C++, the code scv_create runs): it is compiled
with g++ through tests/expected_table_check.cpp, dumped bit for bit, and checked here without a GPU.

* every binomial C(n, i), n <= 256, is float(math.comb(n, i)) or within n * 2^-53 relative of it (the header's claim for Pascal's rule);
* every Gauss-Legendre rule Q = 1 .. 64 has ascending nodes in (0, 1) and positive weights, and integrates y^d on [0, 1] for every
  d <= 2 Q - 1 to within (d + 1) 2^-53 and TABLE_MONOMIAL_BOUND relative of 1 / (d + 1) -- evaluated exactly (integers over a power of two) from the
  stored doubles, so the only error measured is the table's own rounding;
* the CPU mirror's rules (expected._gl01) equal the table bit for bit: both run the same Newton iteration in the x86-64 long double,
  with the same operations in the same order, so no ulp of slack is needed -- and a slack would hide a mirror that drifted back to
  another rule (numpy's leggauss is off by up to 2.2e-12 relative at Q >= 40)."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import expected

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_Q = 64
# Stored nodes and weights are the long double rule rounded once to double (relative 2^-53 each), and y^d carries a node's rounding d
# times, so sum_q w_q y_q^d is within (d + 1) 2^-53 relative of 1 / (d + 1).  Measured on the table: at most 0.5 (d + 1) 2^-53 for every
# (Q, d); the worst in absolute terms is 3.3e-15 (Q = 63, d = 125: nodes near 1 whose rounding y^125 magnifies), pinned below 4e-15.
TABLE_MONOMIAL_BOUND = 4e-15


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("expected_table") / "expected_table_check")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(HERE, "expected_table_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split()
    words, binom_words, max_q = (int(x) for x in out[:3])
    bits = np.array([int(x, 16) for x in out[3:]], dtype=np.uint64)
    assert bits.shape == (words,) and binom_words == 257 * 258 // 2 and max_q == MAX_Q
    assert words == binom_words + MAX_Q * (MAX_Q + 1)
    return bits.view(np.float64), binom_words


def rule(table, Q):
    t, bw = table
    r = t[bw + Q * (Q - 1): bw + Q * (Q - 1) + 2 * Q]
    return r[0::2], r[1::2]


def test_binomials_within_n_ulps_of_the_integers(table):
    t, _ = table
    worst = 0.0
    for n in range(257):
        for i in range(n + 1):
            got, want = float(t[n * (n + 1) // 2 + i]), math.comb(n, i)
            if got != float(want):
                rel = abs(Fraction(got) - want) / want
                assert rel <= Fraction(n, 2 ** 53), (n, i, got, want)
                worst = max(worst, float(rel))
            if n <= 56:                                                  # every C(n, i) < 2^53 is an exact sum of exact terms
                assert got == want, (n, i)
    assert worst > 0.0                                                   # (the rows above 2^53 do round: the bound is exercised)


def test_rules_have_ascending_interior_nodes_and_positive_weights(table):
    for Q in range(1, MAX_Q + 1):
        y, w = rule(table, Q)
        assert np.all((y > 0.0) & (y < 1.0)), Q
        assert np.all(np.diff(y) > 0.0), Q
        assert np.all(w > 0.0), Q
        assert np.allclose(y, 1.0 - y[::-1], rtol=0, atol=2 ** -53) and np.allclose(w, w[::-1], rtol=1e-15, atol=0), Q   # symmetric


def _monomial_errors(y, w):
    """Relative errors |sum_q w_q y_q^d - 1 / (d + 1)| (d + 1), d = 0 .. 2 Q - 1, of the stored doubles, evaluated exactly."""
    ny, ey = zip(*(Fraction(float(v)).as_integer_ratio() for v in y))          # y = ny / ey, ey a power of two
    nw, ew = zip(*(Fraction(float(v)).as_integer_ratio() for v in w))
    sy = [e.bit_length() - 1 for e in ey]
    sw = [e.bit_length() - 1 for e in ew]
    Q = len(y)
    pw = [1] * Q                                                               # ny_q^d
    errs = []
    for d in range(2 * Q):
        shift = [sw[q] + d * sy[q] for q in range(Q)]
        top = max(shift)
        num = sum((nw[q] * pw[q]) << (top - shift[q]) for q in range(Q))         # sum = num / 2^top, exactly
        errs.append(abs(float(Fraction(num * (d + 1) - (1 << top), 1 << top))))
        pw = [pw[q] * ny[q] for q in range(Q)]
    return errs


def test_every_rule_integrates_monomials_of_degree_below_2Q(table):
    worst = (0.0, (0, 0))
    for Q in range(1, MAX_Q + 1):
        y, w = rule(table, Q)
        for d, e in enumerate(_monomial_errors(y, w)):
            assert e <= (d + 1) * 2.0 ** -53 and e <= TABLE_MONOMIAL_BOUND, (Q, d, e)
            worst = max(worst, (e, (Q, d)))
    print("worst monomial error of the table:", worst)


def test_numpy_leggauss_would_not_meet_the_bound():
    # the rule the mirror used before: at Q = 60 it misses the monomials by 2.5e-13 -- the check above is sharp enough to see it
    x, w = np.polynomial.legendre.leggauss(60)
    assert max(_monomial_errors((1.0 + x) / 2.0, w / 2.0)) > 10 * TABLE_MONOMIAL_BOUND


def test_the_mirror_uses_the_tables_rules_bit_for_bit(table):
    for Q in range(1, MAX_Q + 1):
        y, w = rule(table, Q)
        my, mw = expected._gl01(Q)
        assert np.array_equal(my.view(np.uint64), y.view(np.uint64)), Q
        assert np.array_equal(mw.view(np.uint64), w.view(np.uint64)), Q
