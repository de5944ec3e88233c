"""The bootstrap draws of tests/_boot_fuzz.py, without a GPU: on every default seed the two references -- the numpy restatement
tests/independent_bootstrap.py and the C oracle scvo_bootstrap -- agree on the return code and the whole table (r_end = 2^31 - 1 included);
the default seeds reach every stratum the draws are weighted for, by exact conditions; and four wrong bootstraps differ from the right one on
a stated share of the draws, so a kernel with one of those mistakes cannot pass tests/test_gpu_boot_fuzz.py."""
import numpy as np
import pytest

from oracle import coracle
from tests import _boot_fuzz as bf
from tests import independent_bootstrap as ib

SEEDS = range(bf.DEFAULT_SEEDS)
G = np.uint64(0x9E3779B97F4A7C15)


@pytest.fixture(scope="module")
def cases():
    """The default draws with the oracle's (rc, table) of each: computed once, left unchanged."""
    out = []
    for s in SEEDS:
        c = bf.draw(s)
        c.rc, c.want = coracle.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
        c.want.setflags(write=False)
        out.append(c)
    return out


def test_draws_depend_on_the_seed_alone():
    for s in (0, 7, 149):
        a, b = bf.draw(s), bf.draw(s)
        assert bf.describe(a) == bf.describe(b) and a.cells.tobytes() == b.cells.tobytes()
    assert bf.draw(3).cells.tobytes() != bf.draw(4).cells.tobytes()


def test_every_draw_is_a_valid_call_inside_the_work_bounds(cases):
    for c in cases:
        assert c.cells.dtype == coracle.CELL_DTYPE and c.cells.shape == (c.P, c.B) and c.P >= 1 and c.M >= 1, bf.describe(c)
        assert 0 <= c.r_begin <= c.r_end <= bf.R_TOP and c.r_end - c.r_begin == c.R and 0 <= c.seed64 < 2 ** 64, bf.describe(c)
        assert c.B * c.M <= bf.BM_MAX and c.P * c.B * c.R <= bf.WORK and c.R * c.B * c.M <= bf.OUT_WORDS, bf.describe(c)
        hits = c.cells["hit"] == 1
        assert set(np.unique(c.cells["hit"]).tolist()) <= {0, 1} and (c.cells["n_modes"][hits] >= 1).all(), bf.describe(c)
        assert c.overflow == bool((c.cells["n_modes"][hits] >= c.M).any()), bf.describe(c)


def test_the_two_references_agree_on_every_default_seed(cases):
    for c in cases:
        rc, got = ib.bootstrap(c.cells["hit"], c.cells["n_modes"], c.r_begin, c.r_end, c.seed64, c.M)
        assert rc == c.rc and rc in (0, ib.ERR_ARG), (bf.describe(c), rc, c.rc)
        assert got.shape == c.want.shape == (c.R, c.B, c.M) and np.array_equal(got, c.want), bf.describe(c)
        if not c.overflow:
            assert rc == 0, bf.describe(c)


def test_the_default_seeds_reach_every_stratum(cases):
    def some(pred, at_least=1):
        n = sum(1 for c in cases if pred(c))
        assert n >= at_least, n
        return n

    for P in bf.P_EDGES:
        some(lambda c: c.P == P)
    for B in bf.B_EDGES:
        some(lambda c: c.B == B)
    for R in bf.R_EDGES:
        some(lambda c: c.R == R)
    some(lambda c: c.P > 4097 and c.p_kind == "random")
    # both sides of the LDS fit, by the formula of scv_bootstrap restated here
    fit = lambda c: ((c.B * c.M + 3) // 4 * 4) * 4 + ((c.P * c.B + 7) // 8 * 8) * 2       # noqa: E731
    some(lambda c: fit(c) == 144 * 1024 and c.boot_path == 0 and bf.lds_kernel(c))
    some(lambda c: fit(c) == 144 * 1024 - 16 and c.boot_path == 0 and bf.lds_kernel(c))
    some(lambda c: fit(c) > 144 * 1024 and c.boot_path == 0 and not bf.lds_kernel(c) and
         ((c.B * c.M + 3) // 4 * 4) * 4 + (((c.P - 1) * c.B + 7) // 8 * 8) * 2 <= 144 * 1024)           # one row less fits
    some(lambda c: c.B == 1 and c.boot_path == 0 and fit(c) == 144 * 1024 + 16 and (c.P - 1) % 8 == 0)   # exactly one cell above
    some(lambda c: c.boot_path == 3 and fit(c) <= 144 * 1024, 10)                                        # the gather kernel on a table that fits
    # the class bound
    for M in (1, 2, 3, 1025):
        some(lambda c: c.M == M)
    some(lambda c: c.M == c.mmax + 1 and not c.overflow and int(c.cells["n_modes"][c.cells["hit"] == 1].max(initial=0)) == c.mmax)
    some(lambda c: c.M == c.mmax and c.overflow)
    for B, M in bf.BM_PAIRS:
        some(lambda c: (c.B, c.M) == (B, M) and c.R >= 1)
    for mmax in bf.MMAX:
        some(lambda c: not c.overflow and int(c.cells["n_modes"][c.cells["hit"] == 1].max(initial=0)) == min(mmax, c.M - 1) == mmax)
    # the resample range
    some(lambda c: c.r_begin == 0)
    some(lambda c: c.r_begin < 65536 < c.r_end)
    some(lambda c: c.r_begin * c.P < 2 ** 32 <= (c.r_end - 1) * c.P + c.P and c.R >= 2)
    for d in bf.TOP_D:
        some(lambda c: c.r_end == bf.R_TOP - d and c.R >= 1)
    some(lambda c: c.r_end == bf.R_TOP and c.R >= 2 and bf.lds_kernel(c))
    some(lambda c: c.r_end > bf.R_TOP - 256 and c.R >= 2 and not bf.lds_kernel(c))
    for seed64 in (0, 2 ** 64 - 1):
        some(lambda c: c.seed64 == seed64)
    some(lambda c: 0 < c.seed64 < 2 ** 64 - 1, 30)
    # the table
    some(lambda c: not c.cells["hit"].any() and c.M >= 2)
    some(lambda c: (c.cells["hit"] == 1).all() and (c.cells["n_modes"] == 1).all())
    some(lambda c: ((c.cells["hit"] == 0) & (c.cells["n_modes"] >= c.M)).any() and not c.overflow, 20)
    some(lambda c: ((c.cells["hit"] == 0) & (c.cells["n_modes"] == 0)).any())
    some(lambda c: len(np.unique(c.cells["pad"])) > 100 and len(np.unique(c.cells["max_count"])) > 100)
    # both modes; overflow draws whose overflow IS drawn: both references return ERR_ARG (agreement is the test above)
    some(lambda c: c.device, 50)
    some(lambda c: not c.device, 50)
    n = some(lambda c: c.overflow and c.rc == ib.ERR_ARG, len(cases) // 16)
    assert n <= len(cases) // 4
    some(lambda c: c.overflow and c.rc == ib.ERR_ARG and c.device)
    some(lambda c: c.overflow and c.rc == ib.ERR_ARG and not c.device)
    some(lambda c: c.overflow and c.M == 1 and c.B >= 2 and c.rc == ib.ERR_ARG)


# ---- wrong bootstraps ------------------------------------------------------------------------------------------------------------------

def bootstrap_variant(c, wrong=None):
    """The bootstrap written once more, draw by draw as the kernels walk it, with one mistake switched on:
    "short"    the loop ends one resample early (the last row of the table stays zero);
    "m1"       M = 1 and a drawn class-1 hit: counted at counter b * M + 1 (the next budget's class 0) instead of being an overflow --
               scv_bootstrap_lds_k counts class 1 by ballot outside the bound check of the other classes;
    "stride1"  the table indexed idx + b instead of idx * B + b;
    "r16"      r truncated to 16 bits in the generator's argument.
    Returns (rc, int64 [R, B, M])."""
    hit = (c.cells["hit"] != 0).ravel()
    nm = c.cells["n_modes"].astype(np.int64).ravel()
    P, B, M, R = c.P, c.B, c.M, c.R
    out = np.zeros((R, B * M), dtype=np.int64)
    rc = 0
    r_end = c.r_end - (1 if wrong == "short" and R > 0 else 0)
    step = max(1, (1 << 21) // P)
    j = np.arange(P, dtype=np.uint64)[None, :]
    for r0 in range(c.r_begin, r_end, step):
        r = np.arange(r0, min(r_end, r0 + step), dtype=np.uint64)[:, None]
        rows = np.arange(r.shape[0])
        if wrong == "r16":
            r = r & np.uint64(0xFFFF)
        with np.errstate(over="ignore"):
            u = ib.mix64(np.uint64(c.seed64) + G * (r * np.uint64(P) + j + np.uint64(1)))
        idx = (((u >> np.uint64(32)) * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
        for b in range(B):
            cell = idx + b if wrong == "stride1" else idx * B + b
            h, n = hit[cell], nm[cell]
            over = h & (n >= M)
            if wrong == "m1" and M == 1:
                one = h & (n == 1)
                over &= ~one
                if b * M + 1 < B * M:
                    out[r0 - c.r_begin + rows, b * M + 1] += one.sum(axis=1)
            if over.any():
                rc = ib.ERR_ARG
            ok = h & (n < M)
            flat = np.bincount((rows[:, None] * M + np.where(ok, n, 0))[ok], minlength=rows.size * M).reshape(rows.size, M)
            out[r0 - c.r_begin + rows, b * M:(b + 1) * M] += flat
    return rc, out.reshape(R, B, M)


WRONG = ("short", "m1", "stride1", "r16")
MIN_SHARE = 0.10
VARIANT_WORK = 400_000                                                   # the restatement walks draw by draw: the default draws of at most this work


@pytest.fixture(scope="module")
def shares(cases):
    """For every wrong bootstrap, (draws it was run on, draws on which its (rc, table) differs from the oracle's).  "m1" is a mistake of the
    M = 1 calls alone and is measured on those; the three others on every default draw of at most VARIANT_WORK."""
    out = {}
    for wrong in (None,) + WRONG:
        pool = [c for c in cases if (c.M == 1 if wrong == "m1" else c.work <= VARIANT_WORK)]
        diff = 0
        for c in pool:
            rc, got = bootstrap_variant(c, wrong)
            diff += not (rc == c.rc and np.array_equal(got, c.want))
        out[wrong] = (len(pool), diff)
    print("\nwrong-bootstrap shares: " + ", ".join(f"{k}: {d}/{n} = {d / max(n, 1):.0%}" for k, (n, d) in out.items() if k))
    return out


def test_the_restatement_without_a_mistake_is_the_oracle(shares):
    n, diff = shares[None]
    assert n >= bf.DEFAULT_SEEDS // 3 and diff == 0


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_bootstrap_differs_on_a_tenth_of_the_draws(shares, wrong):
    n, diff = shares[wrong]
    print(f"{wrong}: differs on {diff} of {n} draws = {diff / max(n, 1):.1%}")
    assert n >= 10 and diff >= MIN_SHARE * n, (wrong, n, diff)


# ---- the other draws of the GPU file -------------------------------------------------------------------------------------------------------

def test_cu_cases_hold_the_four_counts_inside_the_bounds():
    for cus in (256, 304, 64):
        got = bf.cu_cases(cus)
        assert sorted({c.R for c in got}) == sorted({cus - 1, cus, cus + 1, 2 * cus + 1})
        assert any(c.r_end == bf.R_TOP for c in got)
        for c in got:
            assert bf.lds_kernel(c) and not c.overflow and c.P * c.B * c.R <= bf.WORK and c.R * c.B * c.M <= bf.OUT_WORDS
            assert 0 <= c.r_begin and c.r_end == c.r_begin + c.R <= bf.R_TOP


def test_fused_draws_are_in_the_shapes_of_the_one_launch_form():
    cs = [bf.draw_fused(s) for s in range(24)]
    for c in cs:
        assert 4097 <= c.N <= 6000 and c.P * c.B <= 600 and c.dist in (1, 3, 5) and 1 <= c.R and 0 <= c.r_begin and c.r_end <= bf.R_TOP
    assert sum(c.boot_path == 2 for c in cs) == 12 and sum(c.boot_path == 0 for c in cs) == 12
    assert any(c.r_end == bf.R_TOP and c.boot_path == 0 for c in cs) and any(c.r_end == bf.R_TOP and c.boot_path == 2 for c in cs)
    assert {c.dist for c in cs} == {1, 3, 5}
    # half of the unforced calls select the streaming vote kernel (the one that can hold the bootstrap), two of them ending at 2^31 - 1
    assert sum(c.boot_path == 0 and c.reg_n_max == 4096 for c in cs) == 6 and all(c.reg_n_max == bf.REG_N_MAX for c in cs if c.boot_path == 2)
    assert sum(c.boot_path == 0 and c.reg_n_max == 4096 and c.r_end == bf.R_TOP and c.R >= 2 for c in cs) >= 1
