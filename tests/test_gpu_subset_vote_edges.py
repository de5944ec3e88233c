"""GPU edge tests of the two pool-level entry points, on pools built from explicit class-count profiles (not synth), against their CPU
statements: scv_expected_majority_i32 within 1e-12 relative of the rationals of expected.py (exactly 0.0 where they are 0), and
scv_resample_prefix_i32 bit-exact against resample.py.

* profiles: the max-U pools of tests/test_expected_cpu.py (the Gauss-Legendre rules up to Q = 64), two-way splits 128/128 and 129/127
  with the truth on either side (j up to 128: the tap_hi half of expected_mul, the window down to coefficient -129), 256 distinct votes,
  256 equal votes with the truth present and absent, a truth of 1 and of N - 1 votes, N = 1, 63, 65, 129, 255, and under
  clamp_to_invalid_bin out-of-range votes merging with genuine 1023 votes, truth 1023.  Every budget 0 .. N in calls of at most 32,
  plus one shuffled call with duplicates, negatives and budgets above N; HOST == DEVICE bit for bit, hit_prob=False the same score
  bits, hit_prob >= score, and hit_prob at k = N is the whole-pool hit of scv_aggregate_prefix_i32.
* the persistent grids: 50 mixed problems under the "grid" option 1, 3, 7 give the default grid's bits (both kernels); a HOST call of
  45 000 pools crosses the 64 MiB staging chunk of expected_host, equals one DEVICE launch, and reports a bad vote that only its second
  chunk holds.
* resample: 256 distinct votes at k = 256 (n_modes = 256, tie class 256, M = 257), 256 equal votes (a lane's byte count reaches 256 on
  the last step), the two-way splits, with and without tokens; and one workgroup counting 3 (2^31 - 1) hits of one class (the LDS
  tie table must not wrap at 2^32).
* a seeded count-profile fuzz, 120 draws: N in 1 .. 256, partitions geometric / equal classes / one large class and singletons /
  two-way, distinct random values (some folded onto 1023 under clamp), the truth a class / absent / 1023 / outside the bins, B in
  1 .. 32 ragged budgets, P <= 6, R <= 64; expected against the rationals, resample against the mirror."""
import time

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, expected, resample
from o1_inference_scaling_laws_amd.engine import Engine
from tests.test_expected_cpu import _max_u_pools

pytestmark = pytest.mark.gpu

REL = 1e-12


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.fixture(scope="module")
def clamp_engine():
    eng = Engine(timing=True, clamp_to_invalid_bin=True)
    yield eng
    eng.close()


@pytest.fixture
def grid_option(hip_engine):
    """set_option("grid", g) on the shared engine, restored to the default (0) whatever happens."""
    try:
        yield lambda g: hip_engine.set_option("grid", g)
    finally:
        hip_engine.set_option("grid", 0)


def _shuffled(values, seed):
    row = np.array(values, dtype=np.int64)
    np.random.default_rng(seed).shuffle(row)
    return row.tolist()


def _profiles():
    """name -> (row, truth, clamp): pools of explicit class counts."""
    out = {}
    for i, (row, truth) in enumerate(_max_u_pools()):
        out[f"max_u{i}_N{len(row)}"] = (row, truth, False)
    for a, b in ((128, 128), (129, 127)):
        row = _shuffled([5] * a + [9] * b, a)
        out[f"split_{a}_{b}_truth_a"] = (row, 5, False)
        out[f"split_{a}_{b}_truth_b"] = (row, 9, False)
    distinct = np.random.default_rng(1).permutation(1023)[:256].tolist()
    out["distinct_256"] = (distinct, distinct[17], False)
    out["distinct_256_absent"] = (distinct, next(v for v in range(1023) if v not in set(distinct)), False)
    out["same_256"] = ([77] * 256, 77, False)
    out["same_256_absent"] = ([77] * 256, 78, False)
    geo = sum([[v] * c for v, c in zip((3, 11, 40, 41, 600), (100, 70, 50, 25, 10))], [])      # 255 votes
    out["truth_1_vote"] = (_shuffled(geo + [900], 2), 900, False)
    out["truth_N_minus_1"] = (_shuffled([300] * 255 + [301], 3), 300, False)
    out["truth_absent"] = (_shuffled(geo + [900], 4), 902, False)
    rng = np.random.default_rng(5)
    for N in (1, 63, 65, 129, 255):
        counts = []
        while sum(counts) < N:
            counts.append(min(int(rng.geometric(0.15)), N - sum(counts)))
        vals = rng.permutation(1023)[:len(counts)].tolist()
        row = _shuffled(sum([[v] * c for v, c in zip(vals, counts)], []), N)
        out[f"N{N}"] = (row, vals[int(np.argmax(counts))], False)
    threes = sum([[v] * 3 for v in range(100, 142)], [])
    merged = [1023] * 20 + [-1] * 15 + [1024] * 10 + [5000] * 5 + [7] * 49 + [8] * 30 + threes
    out["clamp_1023_merge"] = (_shuffled(merged, 6), 1023, True)                        # 1023: 20 genuine + 30 clamped votes against 49
    tie = [1023] * 20 + [-1] * 15 + [1024] * 10 + [7] * 45 + [8] * 30 + threes
    out["clamp_1023_tie"] = (_shuffled(tie, 7), 1023, True)                             # 45 votes of 1023 against 45 of 7
    return out


PROFILES = _profiles()
ALL_ROWS = {}                                                                       # (row, truth) -> (E, H) over k = 0 .. N, once per row


def rationals(row, truth):
    key = (tuple(row), truth)
    if key not in ALL_ROWS:
        N = len(row)
        ct, others = expected.row_classes(row, truth)
        ALL_ROWS[key] = expected._exact_row(N, ct, others, list(range(N + 1)))
    return ALL_ROWS[key]


def rel_errors(got, want):
    """Max relative error of got[b] against the rationals want[b]; asserts exact 0.0 where the rational is 0."""
    worst = 0.0
    for b, r in enumerate(want):
        g = float(got[b])
        if r == 0:
            assert g == 0.0, (b, g)
        else:
            worst = max(worst, abs(g - float(r)) / float(r))
    return worst


WORST = {}


@pytest.mark.parametrize("name", list(PROFILES))
def test_expected_profiles_against_the_rationals(hip_engine, clamp_engine, name):
    row, truth, clamp = PROFILES[name]
    eng = clamp_engine if clamp else hip_engine
    N = len(row)
    E, H = rationals(row, truth)
    pool = np.array([row], dtype=np.int32)
    tr = np.array([truth], dtype=np.int32)
    calls = [list(range(k0, min(k0 + 32, N + 1))) for k0 in range(0, N + 1, 32)]
    rng = np.random.default_rng(N + truth)
    calls.append(rng.permutation(rng.integers(-3, N + 8, size=32)).tolist())            # ragged, duplicated, negative, above N
    worst = 0.0
    for nv_list in calls:
        nv = np.array(nv_list, dtype=np.int32)
        ks = np.clip(nv, 0, N).tolist()
        host = eng.expected_majority(pool, tr, nv)
        worst = max(worst, rel_errors(host.score[0], [E[k] for k in ks]), rel_errors(host.hit_prob[0], [H[k] for k in ks]))
        if N in ks:
            host_hit_at_N = host.hit_prob[0, ks.index(N)]
        assert np.all(host.hit_prob >= host.score)
        dp, dtr, dnv = to_dev(pool, tr, nv)
        s, h = eng.expected_majority_device(dp, dtr, dnv)
        eng.sync()
        assert np.array_equal(s.cpu().numpy().view(np.uint64), host.score.view(np.uint64))
        assert np.array_equal(h.cpu().numpy().view(np.uint64), host.hit_prob.view(np.uint64))
        no_hit = eng.expected_majority(pool, tr, nv, hit_prob=False)
        assert no_hit.hit_prob is None and np.array_equal(no_hit.score.view(np.uint64), host.score.view(np.uint64))
    assert worst <= REL, (name, worst)
    WORST[name] = worst
    whole = eng.aggregate_prefix(pool, tr, np.array([N], dtype=np.int32), want_cells=False).tie_class_hits[0]
    full = eng.expected_majority(pool, tr, np.array([N], dtype=np.int32))
    hit = int(whole[1:].sum())                                                            # 0 or 1: the truth among the modes of the pool
    assert (full.hit_prob[0, 0] == 0.0) if hit == 0 else abs(full.hit_prob[0, 0] - 1.0) <= REL
    assert full.hit_prob[0, 0] == host_hit_at_N
    want = sum(whole[m] / m for m in range(1, _lib.TIE_CLASSES) if whole[m])
    assert (full.score[0, 0] == 0.0) if want == 0 else abs(full.score[0, 0] - want) <= REL * want
    if clamp:
        with pytest.raises(_lib.DomainError):
            hip_engine.expected_majority(pool, tr, np.array([1, N], dtype=np.int32))


def test_max_u_pools_report_the_worst_error():
    got = {k: v for k, v in WORST.items() if k.startswith("max_u")}
    if got:
        print("\nworst relative error against the rationals, max-U pools:", max(got.values()), got)


def _mixed_problems(P, N, seed):
    rng = np.random.default_rng(seed)
    rows, truths = [], []
    for _ in range(P):
        row, truth, _bad = _draw_row(rng, N, clamp=False)
        rows.append(row)
        truths.append(truth)
    return np.array(rows, dtype=np.int32), np.array(truths, dtype=np.int32)


def test_expected_grid_option_keeps_the_bits(hip_engine, grid_option):
    pool, tr = _mixed_problems(50, 256, 11)
    nv = np.array([1, 2, 3, 4, 8, 16, 31, 32, 33, 64, 100, 128, 129, 200, 255, 256, 0, 300, -4, 7], dtype=np.int32)
    ref = hip_engine.expected_majority(pool, tr, nv)
    E, H = expected.expected_majority_exact(pool[::7], tr[::7], nv)
    for p in range(len(E)):
        assert rel_errors(ref.score[7 * p], E[p]) <= REL and rel_errors(ref.hit_prob[7 * p], H[p]) <= REL
    dp, dtr, dnv = to_dev(pool, tr, nv)
    for g in (1, 3, 7):
        grid_option(g)
        got = hip_engine.expected_majority(pool, tr, nv)
        s, h = hip_engine.expected_majority_device(dp, dtr, dnv)
        hip_engine.sync()
        for x, y in ((got.score, ref.score), (got.hit_prob, ref.hit_prob), (s.cpu().numpy(), ref.score), (h.cpu().numpy(), ref.hit_prob)):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), g


def test_resample_grid_option_keeps_the_bits(hip_engine, grid_option):
    pool, tr = _mixed_problems(12, 256, 12)
    tok = np.random.default_rng(12).integers(1, 5000, size=pool.shape).astype(np.int32)
    nv = np.array([1, 256, 64, 128, 0, 255, 3], dtype=np.int32)
    want = resample.resample_prefix(pool, tr, nv, 5, 69, seed=3, tokens=tok, M=257)
    for g in (0, 1, 3):
        grid_option(g)
        got = hip_engine.resample_prefix(pool, tr, nv, 64, 3, tokens=tok, r_begin=5, M=257)
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample), g
        assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.truth_count_sum, want.truth_count_sum), g


def test_host_staging_chunks_match_one_device_launch(hip_engine, clamp_engine):
    from o1_inference_scaling_laws_amd import synth
    P, N = 45_000, 256                                                 # expected_host stages 64 MiB / (N * 4 + 4 + 2 * 32 * 8) = 43 577 pools
    a, _t, tr = synth.fill(P, 1, N, 31, 1)
    pool = np.ascontiguousarray(a[:, 0, :])
    nv = np.array(list(range(1, 257, 8)), dtype=np.int32)
    assert nv.shape == (32,)
    host = hip_engine.expected_majority(pool, tr, nv)
    dp, dtr, dnv = to_dev(pool, tr, nv)
    s, h = hip_engine.expected_majority_device(dp, dtr, dnv)
    hip_engine.sync()
    s, h = s.cpu().numpy(), h.cpu().numpy()
    assert np.array_equal(host.score.view(np.uint64), s.view(np.uint64)) and np.array_equal(host.hit_prob.view(np.uint64), h.view(np.uint64))
    sample = [0, 1, 43_576, 43_577, 43_578, 44_999]
    E, H = expected.expected_majority_exact(pool[sample], tr[sample], nv)
    for i, p in enumerate(sample):
        assert rel_errors(host.score[p], E[i]) <= REL and rel_errors(host.hit_prob[p], H[i]) <= REL
    bad = pool.copy()
    bad[44_000, 3] = -2                                                # only the second chunk holds it
    with pytest.raises(_lib.DomainError):
        hip_engine.expected_majority(bad, tr, nv)
    clamped = clamp_engine.expected_majority(bad, tr, nv)
    E, H = expected.expected_majority_exact(bad[44_000:44_001], tr[44_000:44_001], nv)
    assert rel_errors(clamped.score[44_000], E[0]) <= REL and rel_errors(clamped.hit_prob[44_000], H[0]) <= REL
    keep = np.ones(P, dtype=bool)
    keep[44_000] = False
    assert np.array_equal(clamped.score[keep].view(np.uint64), host.score[keep].view(np.uint64))


def _resample_check(eng, pool, tr, nv, R, seed, tokens, M, r0=0, p_off=0):
    want = resample.resample_prefix(pool, tr, nv, r0, r0 + R, seed=seed, tokens=tokens, p_offset=p_off, M=M or None)
    got = eng.resample_prefix(pool, tr, nv, R, seed, tokens=tokens, r_begin=r0, p_offset=p_off, M=M)
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits)
    assert np.array_equal(got.truth_count_sum, want.truth_count_sum)
    if tokens is not None:
        assert np.array_equal(got.token_sum, want.token_sum)
    if M:
        assert np.array_equal(got.per_resample, want.per_resample)
    dp, dt, dtr, dnv = to_dev(pool, tokens, tr, nv)
    tie, ts, tcs, per = eng.resample_prefix_device(dp, dtr, dnv, r0, r0 + R, seed, tokens=dt, p_offset=p_off, M=M if M else None)
    eng.sync()
    assert np.array_equal(tie.cpu().numpy(), want.tie_class_hits) and np.array_equal(tcs.cpu().numpy(), want.truth_count_sum)
    if tokens is not None:
        assert np.array_equal(ts.cpu().numpy(), want.token_sum)
    if M:
        assert np.array_equal(per.cpu().numpy(), want.per_resample)
    return want


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("name", ["distinct_256", "distinct_256_absent", "same_256", "same_256_absent", "split_128_128_truth_a",
                                  "split_128_128_truth_b", "split_129_127_truth_a", "split_129_127_truth_b", "N1", "clamp_1023_merge"])
def test_resample_profiles_bit_exact(hip_engine, clamp_engine, name, tokens):
    row, truth, clamp = PROFILES[name]
    eng = clamp_engine if clamp else hip_engine
    N = len(row)
    pool = np.array([row] * 4, dtype=np.int32)                                          # 4 problems of the same pool: different streams
    tr = np.full(4, truth, dtype=np.int32)
    tok = np.random.default_rng(N).integers(1, 3000, size=pool.shape).astype(np.int32) if tokens else None
    nv = np.array([N, 1, N - 1, 128, 129, 2, N, 0, N + 3], dtype=np.int32)
    want = _resample_check(eng, pool, tr, nv, 64, 9 + N, tok, N + 1, r0=11, p_off=1 << 20)
    if name == "distinct_256":                                                          # every ordering of the whole pool: 256 modes
        assert want.tie_class_hits[0, 256] == 4 * 64 and want.tie_class_hits[0, :256].sum() == 0
    if name == "same_256":
        assert want.tie_class_hits[0, 1] == 4 * 64 and want.truth_count_sum[0] == 4 * 64 * 256


def test_resample_tie_counters_do_not_wrap(hip_engine, grid_option):
    """One workgroup, 3 (2^31 - 1) lanes that all hit with one mode: a 32-bit LDS counter would wrap to 2^31 - 3."""
    R = 2 ** 31 - 1
    pool = np.full((3, 1), 4, dtype=np.int32)
    tr = np.full(3, 4, dtype=np.int32)
    nv = np.array([1], dtype=np.int32)
    dp, dtr, dnv = to_dev(pool, tr, nv)
    grid_option(1)
    t0 = time.perf_counter()
    tie, _ts, tcs, per = hip_engine.resample_prefix_device(dp, dtr, dnv, 0, R, 5)
    hip_engine.sync()
    print(f"\nresample overflow test: {time.perf_counter() - t0:.1f} s")
    tie = tie.cpu().numpy()
    assert per is None
    assert int(tie[0, 1]) == 3 * R and int(tie[0].sum()) == 3 * R
    assert int(tcs.cpu().numpy()[0]) == 3 * R


# ---- a seeded count-profile fuzz ----------------------------------------------------------------------------------------------------

def _partition(rng, N):
    kind = int(rng.integers(0, 4))
    if kind == 0:                                                                         # geometric class sizes
        p = float(rng.uniform(0.02, 0.6))
        counts = []
        while sum(counts) < N:
            counts.append(min(int(rng.geometric(p)), N - sum(counts)))
    elif kind == 1:                                                                       # equal classes (and the remainder)
        s = int(rng.integers(1, N + 1))
        counts = [s] * (N // s) + ([N % s] if N % s else [])
    elif kind == 2:                                                                       # one large class and singletons
        big = int(rng.integers(1, N + 1))
        counts = [big] + [1] * (N - big)
    else:                                                                                 # two-way
        a = int(rng.integers(0, N + 1))
        counts = [c for c in (a, N - a) if c]
    return counts


def _draw_row(rng, N, clamp):
    counts = _partition(rng, N)
    vals = rng.permutation(1023)[:len(counts)].tolist()                                   # distinct values 0 .. 1022
    bad = False
    if clamp and rng.random() < 0.7:                                                      # fold classes onto 1023
        for i in rng.choice(len(counts), size=min(len(counts), int(rng.integers(1, 3))), replace=False).tolist():
            vals[i] = int(rng.choice([1023, -1, 1024, 5000, -77]))
        bad = any(v < 0 or v > 1023 for v in vals)
    row = np.repeat(np.array(vals, dtype=np.int64), counts)
    rng.shuffle(row)
    u = rng.random()
    if u < 0.6:
        truth = int(vals[int(rng.integers(0, len(vals)))])
        truth = 1023 if not 0 <= truth < 1024 else truth
    elif u < 0.8:
        truth = int(next(v for v in rng.permutation(1023).tolist() if v not in set(vals)))     # absent
    elif u < 0.95:
        truth = 1023
    else:
        truth = 4000                                                                      # outside the bins: never hits
    return row.tolist(), truth, bad


FUZZ_DRAWS = 120


@pytest.mark.parametrize("chunk", range(6))
def test_count_profile_fuzz(hip_engine, clamp_engine, chunk):
    for d in range(chunk * FUZZ_DRAWS // 6, (chunk + 1) * FUZZ_DRAWS // 6):
        rng = np.random.default_rng(7000 + d)
        N = int(rng.integers(1, 257)) if d % 4 else int(rng.choice([1, 2, 64, 128, 129, 255, 256]))
        P = int(rng.integers(1, 7))
        clamp = d % 3 == 0
        rows, truths, bads = zip(*(_draw_row(rng, N, clamp) for _ in range(P)))
        pool = np.array(rows, dtype=np.int32)
        tr = np.array(truths, dtype=np.int32)
        B = int(rng.integers(1, 33))
        nv = rng.integers(-2, N + 4, size=B).astype(np.int32)
        if rng.random() < 0.5:
            nv[int(rng.integers(0, B))] = N
        eng = clamp_engine if clamp else hip_engine
        if any(bads):
            with pytest.raises(_lib.DomainError):
                hip_engine.expected_majority(pool, tr, nv)
        E, H = expected.expected_majority_exact(pool, tr, nv)
        if d % 2:
            res = eng.expected_majority(pool, tr, nv)
            score, hit = res.score, res.hit_prob
        else:
            dp, dtr, dnv = to_dev(pool, tr, nv)
            s, h = eng.expected_majority_device(dp, dtr, dnv)
            eng.sync()
            score, hit = s.cpu().numpy(), h.cpu().numpy()
        for p in range(P):
            assert rel_errors(score[p], E[p]) <= REL and rel_errors(hit[p], H[p]) <= REL, (d, p)
        R = int(rng.integers(1, 65))
        tok = rng.integers(0, 4000, size=pool.shape).astype(np.int32) if d % 5 < 2 else None
        kmax = int(np.clip(nv, 0, N).max())
        _resample_check(eng, pool, tr, nv, R, 100 + d, tok, kmax + 1 if d % 2 else 0, r0=int(rng.integers(0, 1000)),
                        p_off=int(rng.integers(0, 1 << 40)))
