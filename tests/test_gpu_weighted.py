"""GPU tests of scv_weighted_prefix_i32 (weighted majority vote and best-of-N over the prefixes of a pool ordering): every output bit-exact
against the CPU mirror (o1_inference_scaling_laws_amd/weighted.py) for both rules and both orders, the reduction to scv_resample_prefix_i32 /
scv_aggregate_prefix_i32 under unit weights, edges (N = 1, 256 equal votes of the largest weight, 256 distinct votes, all-zero rows, every kind
of budget, grids, a HOST call of two chunks, more than 2^32 hits through one workgroup's tie table, empty HOST calls), slices and shards, a captured graph, one timed launch per DEVICE call, and the errors."""
import time

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, curves, synth, weighted
from o1_inference_scaling_laws_amd.engine import Engine, cells_from_torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 8, 16, 63, 64, 65, 127, 128, 129, 200, 255, 256]
RS = [1, 3, 64, 65, 1000]
BS = [1, 8, 32]
WMAX = _lib.WEIGHT_MAX


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.fixture
def grid_option(hip_engine):
    try:
        yield lambda g: hip_engine.set_option("grid", g)
    finally:
        hip_engine.set_option("grid", 0)


def pool_of(P, N, seed, dist):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    return a[:, 0, :].copy(), t[:, 0, :].copy(), tr


def weights_for(pool, seed):
    """Small weights (many ties), planted zeros and WEIGHT_MAX; row 0 all equal, row 1 all zero, row 2 all WEIGHT_MAX (when present)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 6, size=pool.shape)
    big = rng.random(pool.shape) < 0.2
    w[big] = rng.integers(0, WMAX + 1, size=int(big.sum()))
    w[rng.random(pool.shape) < 0.05] = WMAX
    for row, val in ((0, 7), (1, 0), (2, WMAX)):
        if row < pool.shape[0]:
            w[row] = val
    return w.astype(np.int32)


def budgets_for(N, B, seed):
    rng = np.random.default_rng(seed)
    base = [-3, 0, 1, N - 1, N, N + 1, 2 ** 31 - 1] + rng.integers(0, N + 1, size=8).tolist()
    return np.array(rng.choice(base, size=B).tolist(), dtype=np.int32)


def assert_same(got, want, M, cells=False):
    tie, ts, per, c, ct = [None if x is None else x.cpu().numpy() for x in got]
    assert np.array_equal(tie, want.tie_class_hits)
    assert np.array_equal(ts, want.token_sum)
    if M:
        assert np.array_equal(per, want.per_resample)
    if cells:
        assert np.array_equal(cells_from_torch(got[3]), want.cells) and np.array_equal(ct, want.cell_tokens)


def assert_host_same(got, want, M, cells=False):
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits)
    assert (got.token_sum is None and want.token_sum is None) or np.array_equal(got.token_sum, want.token_sum)
    if M:
        assert np.array_equal(got.per_resample, want.per_resample)
    if cells:
        assert np.array_equal(got.cells, want.cells)
        assert (got.cell_tokens is None and want.cell_tokens is None) or np.array_equal(got.cell_tokens, want.cell_tokens)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N, shuffled, rule):
    eng = hip_engine
    for dist in range(6):
        k = NS.index(N) + dist
        B = BS[k % 3]
        R = RS[k % len(RS)] if shuffled else 1
        P = (2 if R >= 1000 else 3 + k % 3) if shuffled else 5 + 7 * (k % 4)
        r0 = (0, 7, 2 ** 31 - 1 - R)[k % 3] if shuffled else 0
        p_off = (0, 5, 1 << 33)[(k + 1) % 3] if shuffled else 0
        seed = 2024 + k
        pool, tok, tr = pool_of(P, N, 40 + k, dist)
        w = weights_for(pool, k)
        nv = budgets_for(N, B, k)
        M = N + 1
        want = weighted.weighted_prefix(pool, w, tr, nv, rule, r0, r0 + R if shuffled else None, seed, p_off, M=M, tokens=tok,
                                        want_cells=not shuffled)
        assert want.error_bits == 0
        dp, dw, dt, dtr, dn = to_dev(pool, w, tok, tr, nv)
        got = eng.weighted_prefix_device(dp, dw, dtr, dn, rule, r0, r0 + R if shuffled else None, seed, p_offset=p_off, tokens=dt, M=M,
                                         want_cells=not shuffled)
        eng.sync()
        assert_same(got, want, M, cells=not shuffled)
        host = eng.weighted_prefix(pool, w, tr, nv, rule, resamples=R if shuffled else None, seed=seed, r_begin=r0, p_offset=p_off, M=M,
                                   tokens=tok, want_cells=not shuffled)
        assert_host_same(host, want, M, cells=not shuffled)


@pytest.mark.parametrize("N", [1, 8, 64, 65, 128, 256])
def test_unit_weights_are_the_plain_vote(hip_engine, N):
    """Every weight 1, rule 0: the shuffled call is scv_resample_prefix_i32, the pool-order call scv_aggregate_prefix_i32 (cells included:
    unit weights make max_count and truth_count counts again)."""
    eng = hip_engine
    pool, tok, tr = pool_of(40, N, N, 1)
    ones = np.ones_like(pool)
    rng = np.random.default_rng(N)
    nv = np.concatenate([[0, 1, N, N], rng.integers(0, N + 1, size=6)]).astype(np.int32)
    for R in (3, 65):                                                   # both row layouts of the kernel
        got = eng.weighted_prefix(pool, ones, tr, nv, 0, resamples=R, seed=3, r_begin=9, p_offset=4, tokens=tok)
        want = eng.resample_prefix(pool, tr, nv, R, 3, tokens=tok, r_begin=9, p_offset=4, M=N + 1)
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
        assert np.array_equal(got.token_sum, want.token_sum)
    cells = eng.weighted_prefix(pool, ones, tr, nv, 0, tokens=tok, want_cells=True)
    ref = eng.aggregate_prefix(pool, tr, nv, tokens=tok, want_cells=True)
    assert np.array_equal(cells.cells, ref.cells) and np.array_equal(cells.cell_tokens, ref.cell_tokens)
    assert np.array_equal(cells.tie_class_hits, ref.tie_class_hits) and np.array_equal(cells.token_sum, ref.token_sum)


@pytest.mark.parametrize("rule", [0, 1])
def test_a_pool_of_one_sample(hip_engine, rule):
    pool = np.array([[5], [6], [7]], dtype=np.int32)
    w = np.array([[3], [0], [WMAX]], dtype=np.int32)
    tr = np.array([5, 6, 8], dtype=np.int32)
    nv = np.array([1, 0, 4], dtype=np.int32)
    for R in (None, 70):
        got = hip_engine.weighted_prefix(pool, w, tr, nv, rule, resamples=R, seed=1, want_cells=R is None)
        want = weighted.weighted_prefix(pool, w, tr, nv, rule, 0, R, 1, M=2, want_cells=R is None)
        assert_host_same(got, want, 2, cells=R is None)
        r = R or 1
        assert got.tie_class_hits[0, 1] == r and got.tie_class_hits[0].sum() == r and not got.tie_class_hits[1].any()
    assert got.token_sum is None


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("rule", [0, 1])
def test_256_equal_and_256_distinct_votes(hip_engine, shuffled, rule):
    """Row 0: 256 votes of one value at WEIGHT_MAX (top = 256 * WEIGHT_MAX < 2^32 under rule 0); row 1: 256 distinct votes of equal weight
    (n_modes = 256 goes to class 256); row 2: every weight 0 (no mode, no hit); row 3: the truth is outside the bins."""
    rng = np.random.default_rng(256)
    pool = np.stack([np.full(256, 17), rng.permutation(1024)[:256], np.full(256, 17), rng.permutation(1024)[:256]]).astype(np.int32)
    tr = np.array([17, int(pool[1, 5]), 17, 2000], dtype=np.int32)
    w = np.stack([np.full(256, WMAX), np.full(256, 9), np.zeros(256), np.full(256, 9)]).astype(np.int32)
    nv = np.array([256, 300, 100, 0], dtype=np.int32)
    R = 16 if shuffled else None
    want = weighted.weighted_prefix(pool, w, tr, nv, rule, 0, R, 9, M=257, want_cells=not shuffled)
    got = hip_engine.weighted_prefix(pool, w, tr, nv, rule, resamples=R, seed=9, M=257, want_cells=not shuffled)
    assert_host_same(got, want, 257, cells=not shuffled)
    r = R or 1
    assert got.tie_class_hits[0, 1] == r and got.tie_class_hits[0, 256] == r and got.tie_class_hits[0].sum() == 2 * r
    if not shuffled:
        assert int(got.cells["max_count"][0, 0]) == (256 * WMAX if rule == 0 else WMAX) and int(got.cells["truth_count"][0, 0]) == int(got.cells["max_count"][0, 0])
        assert int(got.cells["n_modes"][1, 0]) == 256 and int(got.cells["min_mode"][1, 0]) == int(pool[1].min())
        assert (got.cells["max_count"][2] == 0).all() and (got.cells["min_mode"][2] == -1).all() and not got.cells["hit"][2].any()


@pytest.mark.parametrize("rule", [0, 1])
def test_all_zero_weights_never_hit(hip_engine, rule):
    pool, tok, tr = pool_of(7, 50, 5, 2)                                # every vote the truth: any positive weight would hit
    w = np.zeros_like(pool)
    nv = np.array([50, 0, -1, 7, 99], dtype=np.int32)
    for R in (None, 70):
        got = hip_engine.weighted_prefix(pool, w, tr, nv, rule, resamples=R, seed=1, tokens=tok, want_cells=R is None)
        assert not got.tie_class_hits.any() and not got.per_resample.any()
        assert got.token_sum[0] == int(tok.sum()) * (R or 1) and got.token_sum[1] == 0
        if R is None:
            assert (got.cells["max_count"] == 0).all() and (got.cells["min_mode"] == -1).all() and (got.cells["n_modes"] == 0).all()
            assert np.array_equal(got.cell_tokens[:, 0], tok.sum(axis=1))


def test_32_equal_budgets(hip_engine):
    pool, tok, tr = pool_of(20, 128, 3, 1)
    w = weights_for(pool, 3)
    nv = np.full(32, 77, dtype=np.int32)
    for rule in (0, 1):
        got = hip_engine.weighted_prefix(pool, w, tr, nv, rule, resamples=100, seed=2, tokens=tok)
        want = weighted.weighted_prefix(pool, w, tr, nv, rule, 0, 100, 2, M=129, tokens=tok)
        assert_host_same(got, want, 129)
        assert (got.tie_class_hits == got.tie_class_hits[0]).all() and (got.token_sum == got.token_sum[0]).all()


def test_grid_option_keeps_the_bits(hip_engine, grid_option):
    pool, tok, tr = pool_of(12, 256, 12, 3)
    w = weights_for(pool, 12)
    nv = budgets_for(256, 8, 12)
    ref_s = hip_engine.weighted_prefix(pool, w, tr, nv, 0, resamples=64, seed=3, r_begin=5, tokens=tok)
    ref_f = hip_engine.weighted_prefix(pool, w, tr, nv, 1, resamples=5, seed=3, r_begin=5, tokens=tok)
    ref_p = hip_engine.weighted_prefix(pool, w, tr, nv, 1, tokens=tok, want_cells=True)
    for g in (1, 3, 5000):
        grid_option(g)
        assert_host_same(hip_engine.weighted_prefix(pool, w, tr, nv, 0, resamples=64, seed=3, r_begin=5, tokens=tok), ref_s, True)
        assert_host_same(hip_engine.weighted_prefix(pool, w, tr, nv, 1, resamples=5, seed=3, r_begin=5, tokens=tok), ref_f, True)
        assert_host_same(hip_engine.weighted_prefix(pool, w, tr, nv, 1, tokens=tok, want_cells=True), ref_p, True, cells=True)


def test_host_staging_chunks_match_one_device_launch(hip_engine):
    P, N = 30_000, 256                         # pool order with cells: 64 MiB / (3 * 256 * 4 + 4 + 32 * (16 + 8)) = 17 458 pools per chunk
    a, t, tr = synth.fill(P, 1, N, 31, 1, want_tokens=True)
    pool, tok = np.ascontiguousarray(a[:, 0, :]), np.ascontiguousarray(t[:, 0, :])
    w = (1 + (tok % 1000)).astype(np.int32)
    nv = np.arange(8, 264, 8, dtype=np.int32)
    host = hip_engine.weighted_prefix(pool, w, tr, nv, 0, tokens=tok, want_cells=True, M=0)
    dev = hip_engine.weighted_prefix_device(*to_dev(pool, w, tr, nv), 0, tokens=to_dev(tok)[0], want_cells=True)
    hip_engine.sync()
    assert_same(dev, host, 0, cells=True)
    sample = [0, 17_457, 17_458, 29_999]
    want = weighted.weighted_prefix(pool[sample], w[sample], tr[sample], nv, 0, tokens=tok[sample], want_cells=True)
    assert np.array_equal(host.cells[sample], want.cells) and np.array_equal(host.cell_tokens[sample], want.cell_tokens)
    bad = w.copy()
    bad[29_000, 3] = -4                                                 # only the second chunk holds it
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.weighted_prefix(pool, bad, tr, nv, 0, tokens=tok, want_cells=True, M=0)
    assert ei.value.code == _lib.ERR_ARG and "weight" in str(ei.value)


def test_tie_counters_do_not_wrap(hip_engine, grid_option):
    """One workgroup, 3 (2^31 - 1) lanes that all hit with one mode: a 32-bit LDS counter would wrap to 2^31 - 3 (the epoch flush of the tie
    table, as in the sibling bodies)."""
    R = 2 ** 31 - 1
    pool = np.full((3, 1), 4, dtype=np.int32)
    w = np.full((3, 1), 9, dtype=np.int32)
    tok = np.ones((3, 1), dtype=np.int32)
    tr = np.full(3, 4, dtype=np.int32)
    nv = np.array([1], dtype=np.int32)
    grid_option(1)
    t0 = time.perf_counter()
    dp, dw, dt, dtr, dn = to_dev(pool, w, tok, tr, nv)
    tie, ts, per, _, _ = hip_engine.weighted_prefix_device(dp, dw, dtr, dn, 1, 0, R, 5, tokens=dt)
    hip_engine.sync()
    print(f"\nweighted overflow test: {time.perf_counter() - t0:.1f} s")
    tie = tie.cpu().numpy()
    assert per is None
    assert int(tie[0, 1]) == 3 * R and int(tie[0].sum()) == 3 * R and int(ts.cpu().numpy()[0]) == 3 * R


def test_empty_host_calls_overwrite_every_output(hip_engine):
    """HOST mode overwrites every output, per_resample included, also when there is nothing to vote on (P = 0, or an empty range of r)."""
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 8), dtype=np.int32)
    w = np.ones((2, 8), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nv = np.ones(2, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    for P, r0, r1, per_shape in ((0, 0, 3, (3, 2, 4)), (2, 5, 5, (0, 2, 4))):
        tie = np.full((2, 1025), -1, dtype=np.int64)
        sums = np.full(2, -1, dtype=np.int64)
        per = np.full(per_shape, -1, dtype=np.int64)
        have = P > 0
        assert L.scv_weighted_prefix_i32(ctx, ptr(pool) if have else None, ptr(w), ptr(pool), ptr(nv), ptr(tr) if have else None, P, 2, 8, 0,
                                         _lib.RULE_BEST_OF, _lib.ORDER_SHUFFLED, r0, r1, 1, 4, _lib.MEM_HOST, ptr(tie), ptr(sums), ptr(per),
                                         None, None) == _lib.OK
        assert not tie.any() and not sums.any() and not per.any()


def test_slices_and_shards_add_up_on_the_device(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 100, 9, 4)
    w = weights_for(pool, 9)
    nv = budgets_for(100, 6, 9)
    for rule in (0, 1):
        want = weighted.weighted_prefix(pool, w, tr, nv, rule, 3, 203, 11, M=101, tokens=tok)
        dp, dw, dt, dtr, dn = to_dev(pool, w, tok, tr, nv)
        out = eng.weighted_prefix_device(dp, dw, dtr, dn, rule, 3, 80, 11, tokens=dt)
        eng.weighted_prefix_device(dp, dw, dtr, dn, rule, 80, 203, 11, tokens=dt, tie_class_hits=out[0], token_sum=out[1])
        per = torch.zeros((200, 6, 101), dtype=torch.int64, device=dp.device)
        for lo, hi in ((0, 4), (4, 11)):                                # problem shards, each with its global offset
            eng.weighted_prefix_device(dp[lo:hi].contiguous(), dw[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dn, rule, 3, 203, 11,
                                       p_offset=lo, tokens=dt[lo:hi].contiguous(), per_resample=per)
        eng.sync()
        assert_same(out[:2] + (per, None, None), want, 101)
        whole = weighted.weighted_prefix(pool, w, tr, nv, rule, tokens=tok, want_cells=True)
        a = eng.weighted_prefix(pool[:4], w[:4], tr[:4], nv, rule, tokens=tok[:4], want_cells=True)
        b = eng.weighted_prefix(pool[4:], w[4:], tr[4:], nv, rule, tokens=tok[4:], want_cells=True)
        assert np.array_equal(a.tie_class_hits + b.tie_class_hits, whole.tie_class_hits)
        assert np.array_equal(np.concatenate([a.cells, b.cells]), whole.cells)


def test_one_timed_launch_per_device_call(hip_engine):
    pool, tok, tr = pool_of(20, 128, 33, 1)
    w = weights_for(pool, 33)
    nv = budgets_for(128, 8, 33)
    dp, dw, dt, dtr, dn = to_dev(pool, w, tok, tr, nv)
    for kw in (dict(r_end=100), dict(r_end=5), dict(want_cells=True)):
        hip_engine.sync()
        hip_engine.drain_kernel_ns()
        hip_engine.weighted_prefix_device(dp, dw, dtr, dn, 0, 0, seed=4, tokens=dt, M=129, **kw)
        hip_engine.sync()
        ns, launches = hip_engine.drain_kernel_ns()
        assert launches == 1 and ns > 0


def test_host_overwrites_device_accumulates_and_graph():
    import torch
    pool, tok, tr = pool_of(20, 128, 33, 1)
    w = weights_for(pool, 33)
    nv = budgets_for(128, 8, 33)
    want = weighted.weighted_prefix(pool, w, tr, nv, 0, 0, 100, 4, M=129, tokens=tok)
    dp, dw, dt, dtr, dn = to_dev(pool, w, tok, tr, nv)
    with Engine(device=0) as eng:                                       # no SCV_FLAG_TIMING: no event records in the graph
        for _ in range(2):                                              # HOST: the same answer twice, not twice the answer
            assert_host_same(eng.weighted_prefix(pool, w, tr, nv, 0, resamples=100, seed=4, M=129, tokens=tok), want, 129)
        got = eng.weighted_prefix_device(dp, dw, dtr, dn, 0, 0, 100, 4, tokens=dt, M=129)
        eng.weighted_prefix_device(dp, dw, dtr, dn, 0, 0, 100, 4, tokens=dt, tie_class_hits=got[0], token_sum=got[1], per_resample=got[2])
        eng.sync()
        twice = type(want)(want.P, want.R, 2 * want.tie_class_hits, 2 * want.token_sum, 2 * want.per_resample)
        assert_same(got, twice, 129)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got[:3]]
        kw = dict(tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], per_resample=bufs[2])
        with torch.cuda.stream(side):                                   # warm-up on the capture stream
            eng.weighted_prefix_device(dp, dw, dtr, dn, 0, 0, 100, 4, **kw)
        torch.cuda.synchronize()
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.weighted_prefix_device(dp, dw, dtr, dn, 0, 0, 100, 4, **kw)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        eng.sync()
        assert_same(bufs + [None, None], twice, 129)


def test_out_of_domain_votes(hip_engine):
    pool, tok, tr = pool_of(4, 20, 21, 3)
    pool[1, 3], pool[2, 0] = -1, 4096
    tr[2] = 1023
    w = weights_for(pool, 21)
    nv = budgets_for(20, 5, 21)
    with pytest.raises(_lib.DomainError):
        hip_engine.weighted_prefix(pool, w, tr, nv, 0)
    hip_engine.weighted_prefix_device(*to_dev(pool, w, tr, nv), 0, 0, 30, 1)
    with pytest.raises(_lib.DomainError):
        hip_engine.sync()
    want = weighted.weighted_prefix(pool, w, tr, nv, 1, 0, 30, 1, M=21)
    assert want.error_bits & 1
    with Engine(device=0, clamp_to_invalid_bin=True) as ce:
        assert_host_same(ce.weighted_prefix(pool, w, tr, nv, 1, resamples=30, seed=1, M=21), want, 21)
        cells = ce.weighted_prefix(pool, w, tr, nv, 1, want_cells=True)
        assert_host_same(cells, weighted.weighted_prefix(pool, w, tr, nv, 1, want_cells=True), 0, cells=True)


@pytest.mark.parametrize("badw", [-1, WMAX + 1])
def test_a_weight_out_of_range_is_an_argument_error(hip_engine, badw):
    pool, tok, tr = pool_of(4, 20, 22, 1)
    w = weights_for(pool, 22)
    w[3, 19] = badw
    nv = np.array([5, 20], dtype=np.int32)
    assert weighted.weighted_prefix(pool, w, tr, nv).error_bits & weighted.ERR_WEIGHT_BIT
    for R in (None, 7, 70):
        with pytest.raises(_lib.ScvError) as ei:
            hip_engine.weighted_prefix(pool, w, tr, nv, 0, resamples=R)
        assert ei.value.code == _lib.ERR_ARG and "weight" in str(ei.value)
    hip_engine.weighted_prefix_device(*to_dev(pool, w, tr, nv), 1, 0, 7, 1)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    hip_engine.sync()                                                   # the word was cleared: the context is usable
    w[3, 19] = 1
    assert_host_same(hip_engine.weighted_prefix(pool, w, tr, nv, 0, resamples=7, seed=1), weighted.weighted_prefix(pool, w, tr, nv, 0, 0, 7, 1, M=21), 21)


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(8, dtype=np.int32), (3, 1))               # equal weights: the whole pool is an 8-way tie
    w = np.full_like(pool, 5)
    tr = np.array([0, 1, 2], dtype=np.int32)
    nv = np.array([8], dtype=np.int32)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.weighted_prefix(pool, w, tr, nv, 1, resamples=5, M=8)
    assert ei.value.code == _lib.ERR_ARG
    out = hip_engine.weighted_prefix_device(*to_dev(pool, w, tr, nv), 1, 0, 5, 1, M=4)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    assert int(out[0].cpu().numpy()[0, 8]) == 15                        # the tie-class table itself is complete
    hip_engine.sync()


def test_bad_arguments_are_refused_at_the_call(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 300), dtype=np.int32)
    w = np.ones((2, 300), dtype=np.int32)
    tok = np.zeros((2, 300), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nv = np.ones(40, dtype=np.int32)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    cells = np.zeros(600 * 16, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, rule=0, order=1, r0=0, r1=4, p_off=0, M=1, per=None, nvp=nv, tiep=tie, wp=w, tokp=tok, ts=sums, c=None, ct=None):
        return L.scv_weighted_prefix_i32(ctx, ptr(pool), ptr(wp), ptr(tokp), ptr(nvp), ptr(tr), 2, B, N, p_off, rule, order, r0, r1, 1, M,
                                         _lib.MEM_HOST, ptr(tiep), ptr(ts), ptr(per), ptr(c), ptr(ct))
    assert call() == _lib.OK
    assert call(rule=1, order=0, r0=0, r1=1, c=cells, ct=sums) == _lib.OK
    assert call(tokp=None, ts=None) == _lib.OK
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=33), dict(rule=2), dict(rule=-1), dict(order=2), dict(order=-1), dict(order=0),
               dict(order=0, r0=1, r1=2), dict(order=0, r0=0, r1=0), dict(c=cells), dict(ct=sums), dict(r0=5, r1=4), dict(r0=-1),
               dict(p_off=-1), dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(nvp=None), dict(tiep=None), dict(wp=None),
               dict(tokp=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"weighted" in L.scv_last_error(), kw
    with pytest.raises(ValueError):
        hip_engine.weighted_prefix(pool[:, :8], None, tr, nv[:2])
    with pytest.raises(ValueError):
        hip_engine.weighted_prefix(pool[:, :8], w[:, :8], tr, nv[:2], resamples=3, want_cells=True)


def test_the_reference_shape_and_the_curve(hip_engine):
    P, N, R = 30, 128, 1000
    pool, tok, tr = pool_of(P, N, 2025, 1)
    rng = np.random.default_rng(5)
    w = weighted.quantize_weights(rng.random(pool.shape) + 0.5 * (pool == tr[:, None]))       # a verifier that leans to the truth
    limits = [2 ** i for i in range(11, 19)]
    nv = np.array([t // 2 ** 11 for t in limits], dtype=np.int32)
    for rule in (0, 1):
        got = hip_engine.weighted_prefix(pool, w, tr, nv, rule, resamples=R, seed=17, M=0, tokens=tok)
        want = weighted.weighted_prefix(pool, w, tr, nv, rule, 0, R, 17, tokens=tok)
        assert_host_same(got, want, 0)
        recs = curves.weighted_majority_records(hip_engine, pool, w, tr, tok, limits, rule, resamples=R, seed=17)
        assert [r["token_limit"] for r in recs] == limits
        assert [r["accuracy"] for r in recs] == [got.accuracy(b) for b in range(8)]
        assert [r["avg_tokens_used"] for r in recs] == [float(got.avg_tokens_used(b)) for b in range(8)]
        one = curves.weighted_majority_records(hip_engine, pool, w, tr, tok, limits, rule)
        pool_order = weighted.weighted_prefix(pool, w, tr, nv, rule, tokens=tok)
        assert [r["accuracy"] for r in one] == [pool_order.accuracy(b) for b in range(8)]
