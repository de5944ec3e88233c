"""GPU tests of scv_token_budget_prefix_i32 (the majority vote over the longest prefix of a pool ordering that fits a token budget): every
output bit-exact against the CPU mirror (o1_inference_scaling_laws_amd/token_budget.py) in both orders, the reductions to
scv_resample_prefix_i32 / scv_aggregate_prefix_i32 / scv_bootstrap when every sample costs the same, edges (empty prefixes, 256 equal or
distinct votes, 32 equal budgets, grids, a two-chunk HOST call, more than 2^32 hits through one workgroup's tie table), HOST against DEVICE,
slices and shards, a captured graph, the launch counter, and the errors."""
import time

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, curves, synth, token_budget
from o1_inference_scaling_laws_amd.engine import Engine, cells_from_torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 8, 16, 63, 64, 65, 127, 128, 129, 200, 255, 256]
RS = [1, 3, 64, 65, 1000]
BS = [1, 8, 32]


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.fixture
def grid_option(hip_engine):
    try:
        yield lambda g: hip_engine.set_option("grid", g)
    finally:
        hip_engine.set_option("grid", 0)


def pool_of(P, N, seed, dist, zeros=0.1):
    """synth pools and tokens (100 .. 12 000 per sample) with planted zero-token samples (a failed extraction: answer 0, tokens 0)."""
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    pool, tok = a[:, 0, :].copy(), t[:, 0, :].copy()
    z = np.random.default_rng(seed).random(pool.shape) < zeros
    pool[z], tok[z] = 0, 0
    return pool, tok, tr


def budgets_for(tok, B, seed):
    """ragged, unsorted, duplicated: negative, 0, below the first sample, inside the rows, the largest row total, above 2^31."""
    rng = np.random.default_rng(seed)
    tot = int(tok.astype(np.int64).sum(axis=1).max())
    base = [-3, 0, int(tok[:, 0].min()) - 1, tot, tot + 1, 2 ** 31 + 5, 2 ** 40] + rng.integers(0, tot + 1, size=8).tolist()
    return np.array(rng.choice(base, size=B).tolist(), dtype=np.int64)


def assert_same(got, want, M, cells=False):
    tie, ts, vs, tcs, per, c, ct = [None if x is None else x.cpu().numpy() for x in got]
    assert np.array_equal(tie, want.tie_class_hits)
    assert np.array_equal(ts, want.token_sum) and np.array_equal(vs, want.vote_count_sum) and np.array_equal(tcs, want.truth_count_sum)
    if M:
        assert np.array_equal(per, want.per_resample)
    if cells:
        assert np.array_equal(cells_from_torch(got[5]), want.cells) and np.array_equal(ct, want.cell_tokens)


def assert_host_same(got, want, M, cells=False):
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits)
    assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.vote_count_sum, want.vote_count_sum)
    assert np.array_equal(got.truth_count_sum, want.truth_count_sum)
    if M:
        assert np.array_equal(got.per_resample, want.per_resample)
    if cells:
        assert np.array_equal(got.cells, want.cells) and np.array_equal(got.cell_tokens, want.cell_tokens)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N, shuffled):
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
        bud = budgets_for(tok, B, k)
        M = N + 1
        want = token_budget.token_budget_prefix(pool, tok, tr, bud, r0, r0 + R if shuffled else None, seed, p_off, M=M, want_cells=not shuffled)
        assert want.error_bits == 0
        dp, dt, dtr, db = to_dev(pool, tok, tr, bud)
        got = eng.token_budget_prefix_device(dp, dt, dtr, db, r0, r0 + R if shuffled else None, seed, p_offset=p_off, M=M,
                                             want_cells=not shuffled)
        eng.sync()
        assert_same(got, want, M, cells=not shuffled)
        host = eng.token_budget_prefix(pool, tok, tr, bud, resamples=R if shuffled else None, seed=seed, r_begin=r0, p_offset=p_off, M=M,
                                       want_cells=not shuffled)
        assert_host_same(host, want, M, cells=not shuffled)


@pytest.mark.parametrize("N", [1, 8, 64, 65, 128, 256])
def test_equal_tokens_match_the_resample_and_prefix_kernels(hip_engine, N):
    """Every token t and T_b = n_b * t + delta_b: shuffled == scv_resample_prefix_i32 with n_valid = n_b, pool order == scv_aggregate_prefix_i32,
    and the pool-order cell table bootstraps to the counts of the aggregate-prefix table."""
    eng = hip_engine
    t = 13
    pool, _, tr = pool_of(40, N, N, 1, zeros=0.0)
    tok = np.full_like(pool, t)
    rng = np.random.default_rng(N)
    nb = np.concatenate([[0, 1, N, N], rng.integers(0, N + 1, size=6)]).astype(np.int64)
    bud = nb * t + rng.integers(0, t, size=nb.shape)
    nv = nb.astype(np.int32)
    got = eng.token_budget_prefix(pool, tok, tr, bud, resamples=65, seed=3, r_begin=9, p_offset=4)
    want = eng.resample_prefix(pool, tr, nv, 65, 3, tokens=tok, r_begin=9, p_offset=4, M=N + 1)
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
    assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
    assert np.array_equal(got.vote_count_sum, nb * 40 * 65)
    cells = eng.token_budget_prefix(pool, tok, tr, bud, want_cells=True)
    ref = eng.aggregate_prefix(pool, tr, nv, tokens=tok, want_cells=True)
    assert np.array_equal(cells.cells, ref.cells) and np.array_equal(cells.cell_tokens, ref.cell_tokens)
    assert np.array_equal(cells.tie_class_hits, ref.tie_class_hits)
    assert np.array_equal(cells.token_sum, ref.token_sum) and np.array_equal(cells.truth_count_sum, ref.truth_count_sum)
    M = N + 1
    assert np.array_equal(eng.bootstrap(cells.cells, 0, 50, 77, M), eng.bootstrap(ref.cells, 0, 50, 77, M))


def test_budgets_below_the_first_sample_give_empty_prefixes(hip_engine):
    pool, tok, tr = pool_of(7, 50, 5, 2, zeros=0.0)                     # every vote the truth: any non-empty prefix would hit
    bud = np.array([99, 0, -1, 50, 99], dtype=np.int64)                 # every token is >= 100
    for R in (None, 70):
        got = hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=R, seed=1, want_cells=R is None)
        assert not got.tie_class_hits.any() and not got.token_sum.any() and not got.vote_count_sum.any() and not got.truth_count_sum.any()
        assert not got.per_resample.any()
        if R is None:
            assert (got.cells["max_count"] == 0).all() and (got.cells["min_mode"] == -1).all() and not got.cell_tokens.any()


@pytest.mark.parametrize("shuffled", [False, True])
def test_256_equal_and_256_distinct_votes(hip_engine, shuffled):
    rng = np.random.default_rng(256)
    pool = np.stack([np.full(256, 17), rng.permutation(1024)[:256], np.full(256, 17), rng.permutation(1024)[:256]]).astype(np.int32)
    tr = np.array([17, int(pool[1, 5]), 18, 2000], dtype=np.int32)
    tok = rng.integers(0, 5000, size=pool.shape).astype(np.int32)
    bud = np.array([2 ** 40, int(tok.sum(axis=1).max()), 1000, 0], dtype=np.int64)
    R = 16 if shuffled else None
    want = token_budget.token_budget_prefix(pool, tok, tr, bud, 0, R, 9, M=257, want_cells=not shuffled)
    got = hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=R, seed=9, M=257, want_cells=not shuffled)
    assert_host_same(got, want, 257, cells=not shuffled)
    r = R or 1
    assert got.tie_class_hits[0, 1] == r and got.tie_class_hits[0, 256] == r and got.tie_class_hits[0].sum() == 2 * r
    assert got.vote_count_sum[0] == 4 * 256 * r


def test_32_equal_budgets(hip_engine):
    pool, tok, tr = pool_of(20, 128, 3, 1)
    bud = np.full(32, int(tok.astype(np.int64).sum(axis=1).mean()), dtype=np.int64)
    got = hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=100, seed=2)
    want = token_budget.token_budget_prefix(pool, tok, tr, bud, 0, 100, 2, M=129)
    assert_host_same(got, want, 129)
    assert (got.tie_class_hits == got.tie_class_hits[0]).all() and (got.token_sum == got.token_sum[0]).all()


def test_grid_option_keeps_the_bits(hip_engine, grid_option):
    pool, tok, tr = pool_of(12, 256, 12, 3)
    bud = budgets_for(tok, 8, 12)
    ref_s = hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=64, seed=3, r_begin=5)
    ref_p = hip_engine.token_budget_prefix(pool, tok, tr, bud, want_cells=True)
    for g in (1, 3):
        grid_option(g)
        assert_host_same(hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=64, seed=3, r_begin=5), ref_s, True)
        assert_host_same(hip_engine.token_budget_prefix(pool, tok, tr, bud, want_cells=True), ref_p, True, cells=True)


def test_host_staging_chunks_match_one_device_launch(hip_engine):
    P, N = 30_000, 256                         # pool order with cells: 64 MiB / (2 * 256 * 4 + 4 + 32 * (16 + 8)) = 23 797 pools per chunk
    a, t, tr = synth.fill(P, 1, N, 31, 1, want_tokens=True)
    pool, tok = np.ascontiguousarray(a[:, 0, :]), np.ascontiguousarray(t[:, 0, :])
    bud = np.array([2 ** 11 * k for k in range(1, 33)], dtype=np.int64) * 16
    host = hip_engine.token_budget_prefix(pool, tok, tr, bud, want_cells=True)
    dev = hip_engine.token_budget_prefix_device(*to_dev(pool, tok, tr, bud), want_cells=True)
    hip_engine.sync()
    assert_same(dev, host, 0, cells=True)
    sample = [0, 23_796, 23_797, 29_999]
    want = token_budget.token_budget_prefix(pool[sample], tok[sample], tr[sample], bud, want_cells=True)
    assert np.array_equal(host.cells[sample], want.cells) and np.array_equal(host.cell_tokens[sample], want.cell_tokens)
    bad = tok.copy()
    bad[29_000, 3] = -4                                                 # only the second chunk holds it
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.token_budget_prefix(pool, bad, tr, bud)
    assert ei.value.code == _lib.ERR_ARG and "negative" in str(ei.value)


def test_tie_counters_do_not_wrap(hip_engine, grid_option):
    """One workgroup, 3 (2^31 - 1) lanes that all hit with one mode: a 32-bit LDS counter would wrap to 2^31 - 3."""
    R = 2 ** 31 - 1
    pool = np.full((3, 1), 4, dtype=np.int32)
    tok = np.ones((3, 1), dtype=np.int32)
    tr = np.full(3, 4, dtype=np.int32)
    bud = np.array([5], dtype=np.int64)
    grid_option(1)
    t0 = time.perf_counter()
    tie, ts, vs, tcs, per, _, _ = hip_engine.token_budget_prefix_device(*to_dev(pool, tok, tr, bud), 0, R, 5)
    hip_engine.sync()
    print(f"\ntoken-budget overflow test: {time.perf_counter() - t0:.1f} s")
    tie = tie.cpu().numpy()
    assert per is None
    assert int(tie[0, 1]) == 3 * R and int(tie[0].sum()) == 3 * R
    assert int(tcs.cpu().numpy()[0]) == 3 * R and int(ts.cpu().numpy()[0]) == 3 * R and int(vs.cpu().numpy()[0]) == 3 * R


def test_slices_and_shards_add_up_on_the_device(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 100, 9, 4)
    bud = budgets_for(tok, 6, 9)
    want = token_budget.token_budget_prefix(pool, tok, tr, bud, 3, 203, 11, M=101)
    dp, dt, dtr, db = to_dev(pool, tok, tr, bud)
    out = eng.token_budget_prefix_device(dp, dt, dtr, db, 3, 80, 11)
    eng.token_budget_prefix_device(dp, dt, dtr, db, 80, 203, 11, tie_class_hits=out[0], token_sum=out[1], vote_count_sum=out[2],
                                   truth_count_sum=out[3])
    per = torch.zeros((200, 6, 101), dtype=torch.int64, device=dp.device)
    for lo, hi in ((0, 4), (4, 11)):                                    # problem shards, each with its global offset
        eng.token_budget_prefix_device(dp[lo:hi].contiguous(), dt[lo:hi].contiguous(), dtr[lo:hi].contiguous(), db, 3, 203, 11, p_offset=lo,
                                       per_resample=per)
    eng.sync()
    assert_same(out[:4] + (per, None, None), want, 101)
    cells = eng.token_budget_prefix(pool, tok, tr, bud, want_cells=True)
    whole = token_budget.token_budget_prefix(pool, tok, tr, bud, want_cells=True)
    assert_host_same(cells, whole, 0, cells=True)
    a = eng.token_budget_prefix(pool[:4], tok[:4], tr[:4], bud, want_cells=True)
    b = eng.token_budget_prefix(pool[4:], tok[4:], tr[4:], bud, want_cells=True)
    assert np.array_equal(a.tie_class_hits + b.tie_class_hits, whole.tie_class_hits)
    assert np.array_equal(np.concatenate([a.cells, b.cells]), whole.cells)


def test_host_overwrites_device_accumulates_graph_and_stat():
    import torch
    pool, tok, tr = pool_of(20, 128, 33, 1)
    bud = budgets_for(tok, 8, 33)
    want = token_budget.token_budget_prefix(pool, tok, tr, bud, 0, 100, 4, M=129)
    dp, dt, dtr, db = to_dev(pool, tok, tr, bud)
    with Engine(device=0) as eng:                                       # no SCV_FLAG_TIMING: no event records in the graph
        for _ in range(2):                                              # HOST: the same answer twice, not twice the answer
            assert_host_same(eng.token_budget_prefix(pool, tok, tr, bud, resamples=100, seed=4, M=129), want, 129)
        n0 = eng.stat("token_budget_calls")
        assert n0 == 2
        got = eng.token_budget_prefix_device(dp, dt, dtr, db, 0, 100, 4, M=129)
        eng.token_budget_prefix_device(dp, dt, dtr, db, 0, 100, 4, tie_class_hits=got[0], token_sum=got[1], vote_count_sum=got[2],
                                       truth_count_sum=got[3], per_resample=got[4])
        eng.sync()
        assert eng.stat("token_budget_calls") == n0 + 2
        tie, ts, vs, tcs, per = [x.cpu().numpy() for x in got[:5]]
        assert np.array_equal(tie, 2 * want.tie_class_hits) and np.array_equal(per, 2 * want.per_resample)
        assert np.array_equal(ts, 2 * want.token_sum) and np.array_equal(vs, 2 * want.vote_count_sum)
        assert np.array_equal(tcs, 2 * want.truth_count_sum)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got[:5]]
        kw = dict(tie_class_hits=bufs[0], token_sum=bufs[1], vote_count_sum=bufs[2], truth_count_sum=bufs[3], per_resample=bufs[4])
        with torch.cuda.stream(side):                                   # warm-up on the capture stream
            eng.token_budget_prefix_device(dp, dt, dtr, db, 0, 100, 4, **kw)
        torch.cuda.synchronize()
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.token_budget_prefix_device(dp, dt, dtr, db, 0, 100, 4, **kw)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        eng.sync()
        assert_same(bufs + [None, None], type(want)(want.P, want.R, 2 * want.tie_class_hits, 2 * want.token_sum, 2 * want.vote_count_sum,
                                                    2 * want.truth_count_sum, 2 * want.per_resample), 129)


def test_out_of_domain_votes(hip_engine):
    pool, tok, tr = pool_of(4, 20, 21, 3)
    pool[1, 3], pool[2, 0] = -1, 4096
    tr[2] = 1023
    bud = budgets_for(tok, 5, 21)
    with pytest.raises(_lib.DomainError):
        hip_engine.token_budget_prefix(pool, tok, tr, bud)
    hip_engine.token_budget_prefix_device(*to_dev(pool, tok, tr, bud), 0, 30, 1)
    with pytest.raises(_lib.DomainError):
        hip_engine.sync()
    want = token_budget.token_budget_prefix(pool, tok, tr, bud, 0, 30, 1, M=21)
    assert want.error_bits & 1
    with Engine(device=0, clamp_to_invalid_bin=True) as ce:
        assert_host_same(ce.token_budget_prefix(pool, tok, tr, bud, resamples=30, seed=1, M=21), want, 21)
        cells = ce.token_budget_prefix(pool, tok, tr, bud, want_cells=True)
        assert_host_same(cells, token_budget.token_budget_prefix(pool, tok, tr, bud, want_cells=True), 0, cells=True)


def test_negative_tokens_are_an_argument_error(hip_engine):
    pool, tok, tr = pool_of(4, 20, 22, 1)
    tok[3, 19] = -1
    bud = np.array([5000, 10 ** 6], dtype=np.int64)
    for R in (None, 7):
        with pytest.raises(_lib.ScvError) as ei:
            hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=R)
        assert ei.value.code == _lib.ERR_ARG
    hip_engine.token_budget_prefix_device(*to_dev(pool, tok, tr, bud), 0, 7, 1)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    hip_engine.sync()                                                   # the word was cleared


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(8, dtype=np.int32), (3, 1))               # the whole pool is an 8-way tie
    tok = np.ones_like(pool)
    tr = np.array([0, 1, 2], dtype=np.int32)
    bud = np.array([8], dtype=np.int64)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=5, M=8)
    assert ei.value.code == _lib.ERR_ARG
    out = hip_engine.token_budget_prefix_device(*to_dev(pool, tok, tr, bud), 0, 5, 1, M=4)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    assert int(out[0].cpu().numpy()[0, 8]) == 15                        # the tie-class table itself is complete
    hip_engine.sync()


def test_bad_arguments_are_refused_at_the_call(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 300), dtype=np.int32)
    tok = np.zeros((2, 300), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    bud = np.ones(40, dtype=np.int64)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    cells = np.zeros(600 * 16, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, order=1, r0=0, r1=4, p_off=0, M=1, per=None, budp=bud, tiep=tie, tokp=tok, c=None, ct=None):
        return L.scv_token_budget_prefix_i32(ctx, ptr(pool), ptr(tokp), ptr(budp), ptr(tr), 2, B, N, p_off, order, r0, r1, 1, M, _lib.MEM_HOST,
                                             ptr(tiep), ptr(sums), ptr(sums), ptr(sums), ptr(per), ptr(c), ptr(ct))
    assert call() == _lib.OK
    assert call(order=0, r0=0, r1=1, c=cells, ct=sums) == _lib.OK
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=33), dict(order=2), dict(order=-1), dict(order=0), dict(order=0, r0=1, r1=2),
               dict(order=0, r0=0, r1=0), dict(c=cells), dict(ct=sums), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1),
               dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(budp=None), dict(tiep=None), dict(tokp=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"token_budget" in L.scv_last_error(), kw


def test_the_reference_shape_and_the_curve(hip_engine):
    P, N, R = 30, 128, 1000
    pool, tok, tr = pool_of(P, N, 2025, 1, zeros=0.0)
    limits = [2 ** i for i in range(11, 19)]
    bud = np.array(limits, dtype=np.int64)
    got = hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=R, seed=17, M=0)
    want = token_budget.token_budget_prefix(pool, tok, tr, bud, 0, R, 17)
    assert_host_same(got, want, 0)
    recs = curves.token_budget_records(hip_engine, pool, tr, tok, limits, resamples=R, seed=17)
    assert [r["accuracy"] for r in recs] == [got.accuracy(b) for b in range(8)]
    assert [r["avg_tokens_used"] for r in recs] == [float(got.avg_tokens_used(b)) for b in range(8)]
    assert all(r["avg_tokens_used"] <= r["token_limit"] for r in recs)
    one = curves.token_budget_records(hip_engine, pool, tr, tok, limits)
    pool_order = token_budget.token_budget_prefix(pool, tok, tr, bud)
    assert [r["accuracy"] for r in one] == [pool_order.accuracy(b) for b in range(8)]


@pytest.mark.parametrize("N", [185, 186, 188])
def test_many_budgets_on_64_lane_workgroups(hip_engine, N):
    """Shuffled, R = 1, B = 22: the workgroup that keeps the most lanes resident is of 64 lanes, fewer than the 3 B = 66 per-budget LDS sums
    it must clear before counting (vote sums of budgets 20 and 21 once kept what an earlier workgroup had left in LDS)."""
    pool, tok, tr = pool_of(2000, N, N, 1)
    bud = budgets_for(tok, 22, N)
    dp, dt, dtr, db = to_dev(pool, tok, tr, bud)
    for seed in (1, 2):
        want = token_budget.token_budget_prefix(pool, tok, tr, bud, 0, 1, seed, M=N + 1)
        got = hip_engine.token_budget_prefix_device(dp, dt, dtr, db, 0, 1, seed, M=N + 1)
        hip_engine.sync()
        assert_same(got, want, N + 1)
        assert_host_same(hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=1, seed=seed, M=N + 1), want, N + 1)


def test_empty_host_calls_overwrite_per_resample(hip_engine):
    """HOST mode overwrites every output, per_resample included, also when there is nothing to vote on (P = 0)."""
    L, ctx = _lib.load(), hip_engine._ctx
    bud = np.ones(2, dtype=np.int64)
    nv = np.ones(2, dtype=np.int32)
    tie = np.full((2, 1025), -1, dtype=np.int64)
    sums = np.full(2, -1, dtype=np.int64)
    per = np.full((3, 2, 4), -1, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    assert L.scv_token_budget_prefix_i32(ctx, None, None, ptr(bud), None, 0, 2, 8, 0, _lib.ORDER_SHUFFLED, 0, 3, 1, 4, _lib.MEM_HOST,
                                         ptr(tie), ptr(sums), ptr(sums), ptr(sums), ptr(per), None, None) == _lib.OK
    assert not tie.any() and not sums.any() and not per.any()
    tie[:], sums[:], per[:] = -1, -1, -1
    assert L.scv_resample_prefix_i32(ctx, None, None, ptr(nv), None, 0, 2, 8, 0, 0, 3, 1, 4, _lib.MEM_HOST, ptr(tie), None, ptr(sums),
                                     ptr(per)) == _lib.OK
    assert not tie.any() and not sums.any() and not per.any()
