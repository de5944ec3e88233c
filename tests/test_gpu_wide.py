"""GPU tests of scv_resample_wide_i32 (expected majority vote over sorted random orderings of pools of up to 4096 samples): every output
bit-exact against the CPU mirror (o1_inference_scaling_laws_amd/wide.py) across the pad boundaries of the sort and the workgroup-size
steps, many items per workgroup, accumulation / overwrite, slices and shards, a fresh context, a captured graph, the whole-pool identity
against scv_aggregate_prefix_i32, errors, and 100 random draws of shape and options."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, curves, synth, wide
from tests.test_gpu_resample import budgets_for

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2049, 4095, 4096]
RS = [1, 3, 5, 65]


def pool_of(P, N, seed, dist, tokens):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=tokens)
    return a[:, 0, :].copy(), (t[:, 0, :].copy() if tokens else None), tr


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def assert_same(got, want, tokens, M, times=1):
    tie, tok, tcs, per = [None if x is None else x.cpu().numpy() for x in got]
    assert np.array_equal(tie, times * want.tie_class_hits)
    assert np.array_equal(tcs, times * want.truth_count_sum)
    if tokens:
        assert np.array_equal(tok, times * want.token_sum)
    if M:
        assert np.array_equal(per, times * want.per_resample)


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N, tokens):
    eng = hip_engine
    for dist in range(6):
        k = NS.index(N) + dist
        R = RS[k % len(RS)]
        P = 2 + (k % 4)
        r0 = (0, 7, 2 ** 31 - 1 - R)[k % 3]
        p_off = (0, 5, 1 << 33)[(k + 1) % 3]
        nv = np.array(budgets_for(N, k % 3), dtype=np.int32)
        pool, tok, tr = pool_of(P, N, 40 + k, dist, tokens)
        kmax = int(np.clip(nv, 0, N).max())
        M = kmax + 1
        want = wide.resample_wide(pool, tr, nv, r0, r0 + R, seed=2024 + k, tokens=tok, p_offset=p_off, M=M)
        dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
        got = eng.resample_wide_device(dp, dtr, dnv, r0, r0 + R, 2024 + k, tokens=dt, p_offset=p_off, M=M)
        eng.sync()
        assert_same(got, want, tokens, M)


@pytest.mark.parametrize("grid", [1, 7])
def test_many_items_per_workgroup_across_problem_boundaries(grid):
    """A small forced grid: every workgroup walks a long run of items, over the ends of problems (200 items each)."""
    from o1_inference_scaling_laws_amd.engine import Engine
    P, R, N = 3, 200, 300
    pool, tok, tr = pool_of(P, N, 77, 1, True)
    nv = np.array([1, 2, 4, 8, 150, 300, 299, 0], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 4, 4 + R, seed=8, tokens=tok, M=301)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    with Engine(device=0) as eng:
        eng.set_option("grid", grid)
        got = eng.resample_wide_device(dp, dtr, dnv, 4, 4 + R, 8, tokens=dt, M=301)
        eng.sync()
        assert_same(got, want, True, 301)
        res = eng.resample_wide(pool, tr, nv, R, 8, tokens=tok, r_begin=4, M=301)
        assert np.array_equal(res.tie_class_hits, want.tie_class_hits) and np.array_equal(res.per_resample, want.per_resample)
        assert np.array_equal(res.token_sum, want.token_sum) and np.array_equal(res.truth_count_sum, want.truth_count_sum)


def test_host_mode_overwrites_and_device_mode_accumulates(hip_engine):
    eng = hip_engine
    pool, tok, tr = pool_of(9, 700, 3, 1, True)
    nv = np.array([1, 2, 4, 8, 16, 32, 700], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 0, 30, seed=5, tokens=tok, M=701)
    for _ in range(2):                                                     # HOST: the same answer twice, not twice the answer
        got = eng.resample_wide(pool, tr, nv, 30, 5, tokens=tok, M=701)
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
        assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
        assert got.accuracy(3) == want.accuracy(3) and got.exact_accuracy(6) == want.exact_accuracy(6)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    bufs = eng.resample_wide_device(dp, dtr, dnv, 0, 30, 5, tokens=dt, M=701)
    eng.resample_wide_device(dp, dtr, dnv, 0, 30, 5, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2],
                             per_resample=bufs[3])
    eng.sync()
    assert_same(bufs, want, True, 701, times=2)


def test_slices_and_shards_add_up_on_the_device(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 530, 9, 4, True)
    nv = np.array([530, 1, 64, 7, 300], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 3, 53, seed=11, tokens=tok, M=531)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    tie, ts, tcs, _ = eng.resample_wide_device(dp, dtr, dnv, 3, 20, 11, tokens=dt)
    eng.resample_wide_device(dp, dtr, dnv, 20, 53, 11, tokens=dt, tie_class_hits=tie, token_sum=ts, truth_count_sum=tcs)
    per = torch.zeros((50, 5, 531), dtype=torch.int64, device=dp.device)
    for lo, hi in ((0, 4), (4, 11)):                                       # problem shards, each with its global offset
        eng.resample_wide_device(dp[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dnv, 3, 53, 11, tokens=dt[lo:hi].contiguous(),
                                 p_offset=lo, per_resample=per)
    eng.sync()
    assert np.array_equal(tie.cpu().numpy(), want.tie_class_hits)
    assert np.array_equal(ts.cpu().numpy(), want.token_sum) and np.array_equal(tcs.cpu().numpy(), want.truth_count_sum)
    assert np.array_equal(per.cpu().numpy(), want.per_resample)


def test_first_call_of_a_fresh_context_and_a_captured_graph():
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    pool, tok, tr = pool_of(6, 1500, 33, 1, True)
    nv = np.array([1 << k for k in range(11)] + [1500], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 0, 40, seed=4, tokens=tok, M=1501)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    with Engine(device=0) as eng:                                          # no SCV_FLAG_TIMING: no event records in the graph
        got = eng.resample_wide_device(dp, dtr, dnv, 0, 40, 4, tokens=dt, M=1501)
        eng.sync()
        assert_same(got, want, True, 1501)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got]
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
            eng.resample_wide_device(dp, dtr, dnv, 0, 40, 4, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1],
                                     truth_count_sum=bufs[2], per_resample=bufs[3])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.resample_wide_device(dp, dtr, dnv, 0, 40, 4, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1],
                                     truth_count_sum=bufs[2], per_resample=bufs[3])
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g.replay()
        g.replay()                                                         # replayed twice: DEVICE mode accumulates
        torch.cuda.synchronize()
        eng.sync()
        assert_same(bufs, want, True, 1501, times=2)


@pytest.mark.parametrize("N", [8, 256, 700, 4096])
def test_whole_pool_budgets_are_R_times_the_prefix_call(hip_engine, N):
    eng = hip_engine
    pool, tok, tr = pool_of(12, N, 13, 1, True)
    nv = np.array([N, N + 1, N], dtype=np.int32)
    R = 9
    got = eng.resample_wide(pool, tr, nv, R, 77, tokens=tok, r_begin=1000, M=0)
    ref = eng.aggregate_prefix(pool, tr, nv, tokens=tok, want_cells=False)
    assert got.per_resample is None
    assert np.array_equal(got.tie_class_hits, R * ref.tie_class_hits)
    assert np.array_equal(got.token_sum, R * ref.token_sum) and np.array_equal(got.truth_count_sum, R * ref.truth_count_sum)
    assert got.accuracy(0) == ref.accuracy(0)


def test_out_of_domain_votes(hip_engine):
    from o1_inference_scaling_laws_amd.engine import Engine
    pool, _, tr = pool_of(4, 520, 21, 3, False)
    pool[1, 3], pool[2, 0], pool[3, 519] = -1, 4096, 1024
    tr[2] = 1023
    nv = np.array([1, 5, 520], dtype=np.int32)
    with pytest.raises(_lib.DomainError):
        hip_engine.resample_wide(pool, tr, nv, 10, 1)
    dp, dtr, dnv = to_dev(pool, tr, nv)
    hip_engine.resample_wide_device(dp, dtr, dnv, 0, 10, 1)
    with pytest.raises(_lib.DomainError):
        hip_engine.sync()
    want = wide.resample_wide(pool, tr, nv, 0, 10, seed=1, M=521)
    assert want.error_bits & 1
    with Engine(device=0, clamp_to_invalid_bin=True) as ce:
        got = ce.resample_wide(pool, tr, nv, 10, 1, M=521)
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
        assert np.array_equal(got.truth_count_sum, want.truth_count_sum)


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(300, dtype=np.int32), (3, 1))                # every prefix is an all-way tie: n_modes == k
    tr = np.array([0, 1, 2], dtype=np.int32)
    nv = np.array([300], dtype=np.int32)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.resample_wide(pool, tr, nv, 5, 1, M=300)
    assert ei.value.code == _lib.ERR_ARG
    dp, dtr, dnv = to_dev(pool, tr, nv)
    tie, _, _, _ = hip_engine.resample_wide_device(dp, dtr, dnv, 0, 5, 1, M=4)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    assert int(tie.cpu().numpy()[0, 300]) == 15                             # the tie-class table itself is complete (class 300: beyond the LDS table)
    hip_engine.sync()                                                      # the word was cleared


def test_bad_shapes_are_refused_at_the_call(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 4100), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nv = np.ones(40, dtype=np.int32)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, r0=0, r1=4, p_off=0, M=1, tok=None, tok_out=None, per=None, nvp=nv, tiep=tie):
        return L.scv_resample_wide_i32(ctx, ptr(pool), ptr(tok), ptr(nvp), ptr(tr), 2, B, N, p_off, r0, r1, 1, M, _lib.MEM_HOST,
                                       ptr(tiep), ptr(tok_out), ptr(sums), ptr(per))
    assert call() == _lib.OK
    assert call(N=4096) == _lib.OK
    for kw in (dict(N=0), dict(N=4097), dict(B=0), dict(B=33), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1),
               dict(tok_out=sums), dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(nvp=None), dict(tiep=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"resample_wide" in L.scv_last_error(), kw


def test_the_curve_records(hip_engine):
    pool, tok, tr = pool_of(5, 1024, 2025, 1, True)
    limits = [2 ** i for i in range(11, 22)]
    recs = curves.wide_majority_records(hip_engine, pool, tr, tok, limits, 20, 17)
    want = wide.resample_wide(pool, tr, [1 << k for k in range(11)], 0, 20, seed=17, tokens=tok)
    assert [r["token_limit"] for r in recs] == limits
    assert [r["accuracy"] for r in recs] == [want.accuracy(b) for b in range(11)]
    assert [r["avg_tokens_used"] for r in recs] == [float(want.avg_tokens_used(b)) for b in range(11)]


FUZZ_N_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600)


def fuzz_draw(seed):
    """One valid call that depends on the seed alone: shape, pool kind, budgets, mode and options (N <= 600, P * R * N <= 150 000)."""
    rng = np.random.default_rng((7_300_000, seed))
    N = int(rng.choice(FUZZ_N_EDGES)) if rng.random() < 0.5 else int(rng.integers(1, 601))
    B = int(rng.choice((1, 2, 31, 32))) if rng.random() < 0.3 else int(rng.integers(1, 33))
    R = int(rng.choice((1, 2, 3, 64, 65))) if rng.random() < 0.4 else int(rng.integers(1, 41))
    P = int(rng.integers(1, 7))
    while P * R * N > 150_000 and R > 1:
        R = max(1, R // 2)
    tokens = bool(rng.random() < 0.6)
    pool, tok, tr = pool_of(P, N, 31_000 + seed, int(rng.integers(0, 6)), tokens)
    fold = int(rng.choice([2, 3, 5, 40])) if rng.random() < 0.4 else 0
    if fold:                                                               # few bins: heavy ties
        pool, tr = pool % fold, (tr % fold).astype(np.int32)
    if seed % 10 == 7:                                                     # min(N, 1024) distinct bins per row: the largest tie classes
        pool = np.stack([rng.permutation(1024)[np.arange(N) % 1024] for _ in range(P)]).astype(np.int32)
        tr = pool[:, 0].copy()
    if rng.random() < 0.3:
        tr[:: int(rng.integers(1, 4))] = int(rng.choice((1023, -3, 2000)))
    edges = [-3, 0, 1, N - 1, N, N + 1]
    nv = np.array([int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(0, N + 2)) for _ in range(B)], dtype=np.int32)
    kmax = int(np.clip(nv, 0, N).max())
    return dict(P=P, N=N, B=B, R=R, pool=np.ascontiguousarray(pool.astype(np.int32)), tok=tok, tr=tr.astype(np.int32), nv=nv,
                r0=int(rng.choice((0, 7, 2 ** 31 - 1 - R))), p_off=int(rng.choice((0, 5, 1 << 33))), seed=int(rng.integers(0, 2 ** 63)),
                M=(None if rng.random() < 0.3 else kmax + 1), device=bool(rng.random() < 0.5),
                grid=(int(rng.integers(1, 9)) if rng.random() < 0.4 else 0))


@pytest.mark.parametrize("part", range(4))
def test_fuzz_100_draws(part):
    from o1_inference_scaling_laws_amd.engine import Engine
    with Engine(device=0) as eng:
        for seed in range(25 * part, 25 * part + 25):
            c = fuzz_draw(seed)
            want = wide.resample_wide(c["pool"], c["tr"], c["nv"], c["r0"], c["r0"] + c["R"], seed=c["seed"], tokens=c["tok"],
                                      p_offset=c["p_off"], M=c["M"])
            assert want.error_bits == 0
            eng.set_option("grid", c["grid"])
            what = {k: v for k, v in c.items() if k not in ("pool", "tok", "tr")}
            if c["device"]:
                dp, dt, dtr, dnv = to_dev(c["pool"], c["tok"], c["tr"], c["nv"])
                got = eng.resample_wide_device(dp, dtr, dnv, c["r0"], c["r0"] + c["R"], c["seed"], tokens=dt, p_offset=c["p_off"], M=c["M"])
                eng.sync()
                tie, tok, tcs, per = [None if x is None else x.cpu().numpy() for x in got]
            else:
                res = eng.resample_wide(c["pool"], c["tr"], c["nv"], c["R"], c["seed"], tokens=c["tok"], r_begin=c["r0"], p_offset=c["p_off"],
                                        M=c["M"] or 0)
                tie, tok, tcs, per = res.tie_class_hits, res.token_sum, res.truth_count_sum, res.per_resample
            assert np.array_equal(tie, want.tie_class_hits), what
            assert np.array_equal(tcs, want.truth_count_sum), what
            if c["tok"] is not None:
                assert np.array_equal(tok, want.token_sum), what
            if c["M"]:
                assert np.array_equal(per, want.per_resample), what
