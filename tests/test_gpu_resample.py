"""GPU tests of scv_resample_prefix_i32 (expected majority vote over random pool orderings): every output bit-exact against the
CPU mirror (o1_inference_scaling_laws_amd/resample.py), accumulation / overwrite, slices and shards, the whole-pool identity against
scv_aggregate_prefix_i32, errors, a fresh context, a captured graph, and the reference's own shape."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, curves, resample, synth

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 8, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200, 255, 256]
RS = [1, 3, 64, 65, 1000]


def budgets_for(N, variant):
    ref = [1 << k for k in range(N.bit_length()) if (1 << k) <= N]
    if variant == 0:
        return ref                                                         # the reference's 1, 2, 4 ... (o1.py:274-277)
    if variant == 1:
        return ref[::-1] + [N, 0, N + 5]                                   # unsorted, the whole pool, empty, beyond the pool
    rng = np.random.default_rng(N)
    return rng.integers(-2, N + 3, size=32).tolist()                      # ragged, duplicated, B = 32


def pool_of(P, N, seed, dist, tokens):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=tokens)
    return a[:, 0, :].copy(), (t[:, 0, :].copy() if tokens else None), tr


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def assert_same(got, want, tokens, M):
    tie, tok, tcs, per = [None if x is None else x.cpu().numpy() for x in got]
    assert np.array_equal(tie, want.tie_class_hits)
    assert np.array_equal(tcs, want.truth_count_sum)
    if tokens:
        assert np.array_equal(tok, want.token_sum)
    if M:
        assert np.array_equal(per, want.per_resample)


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N, tokens):
    eng = hip_engine
    for dist in range(6):
        k = NS.index(N) + dist
        R = RS[k % len(RS)]
        P = 2 if R >= 1000 else 3 + (k % 3)
        r0 = (0, 7, 2 ** 31 - 1 - R)[k % 3]
        p_off = (0, 5, 1 << 33)[(k + 1) % 3]
        nv = np.array(budgets_for(N, k % 3), dtype=np.int32)
        pool, tok, tr = pool_of(P, N, 40 + k, dist, tokens)
        kmax = int(np.clip(nv, 0, N).max())
        M = kmax + 1
        want = resample.resample_prefix(pool, tr, nv, r0, r0 + R, seed=2024 + k, tokens=tok, p_offset=p_off, M=M)
        dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
        got = eng.resample_prefix_device(dp, dtr, dnv, r0, r0 + R, 2024 + k, tokens=dt, p_offset=p_off, M=M)
        eng.sync()
        assert_same(got, want, tokens, M)


def test_host_mode_overwrites_and_device_mode_accumulates(hip_engine):
    eng = hip_engine
    pool, tok, tr = pool_of(9, 40, 3, 1, True)
    nv = np.array([1, 2, 4, 8, 16, 32, 40], dtype=np.int32)
    want = resample.resample_prefix(pool, tr, nv, 0, 70, seed=5, tokens=tok, M=41)
    for _ in range(2):                                                     # HOST: the same answer twice, not twice the answer
        got = eng.resample_prefix(pool, tr, nv, 70, 5, tokens=tok, M=41)
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
        assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
        assert got.accuracy(3) == want.accuracy(3) and got.exact_accuracy(6) == want.exact_accuracy(6)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    bufs = eng.resample_prefix_device(dp, dtr, dnv, 0, 70, 5, tokens=dt, M=41)
    eng.resample_prefix_device(dp, dtr, dnv, 0, 70, 5, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2],
                               per_resample=bufs[3])
    eng.sync()
    assert np.array_equal(bufs[0].cpu().numpy(), 2 * want.tie_class_hits)
    assert np.array_equal(bufs[1].cpu().numpy(), 2 * want.token_sum)
    assert np.array_equal(bufs[2].cpu().numpy(), 2 * want.truth_count_sum)
    assert np.array_equal(bufs[3].cpu().numpy(), 2 * want.per_resample)


def test_slices_and_shards_add_up_on_the_device(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 100, 9, 4, True)
    nv = np.array([100, 1, 64, 7, 32], dtype=np.int32)
    want = resample.resample_prefix(pool, tr, nv, 3, 203, seed=11, tokens=tok, M=101)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    tie, ts, tcs, _ = eng.resample_prefix_device(dp, dtr, dnv, 3, 80, 11, tokens=dt)
    eng.resample_prefix_device(dp, dtr, dnv, 80, 203, 11, tokens=dt, tie_class_hits=tie, token_sum=ts, truth_count_sum=tcs)
    per = torch.zeros((200, 5, 101), dtype=torch.int64, device=dp.device)
    for lo, hi in ((0, 4), (4, 11)):                                       # problem shards, each with its global offset
        eng.resample_prefix_device(dp[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dnv, 3, 203, 11, tokens=dt[lo:hi].contiguous(),
                                   p_offset=lo, per_resample=per)
    eng.sync()
    assert np.array_equal(tie.cpu().numpy(), want.tie_class_hits)
    assert np.array_equal(ts.cpu().numpy(), want.token_sum) and np.array_equal(tcs.cpu().numpy(), want.truth_count_sum)
    assert np.array_equal(per.cpu().numpy(), want.per_resample)


@pytest.mark.parametrize("N", [8, 64, 128, 256])
def test_whole_pool_budgets_are_R_times_the_prefix_call(hip_engine, N):
    eng = hip_engine
    pool, tok, tr = pool_of(50, N, 13, 1, True)
    nv = np.array([N, N + 1, N], dtype=np.int32)
    R = 37
    got = eng.resample_prefix(pool, tr, nv, R, 77, tokens=tok, r_begin=1000, M=0)
    ref = eng.aggregate_prefix(pool, tr, nv, tokens=tok, want_cells=False)
    assert got.per_resample is None
    assert np.array_equal(got.tie_class_hits, R * ref.tie_class_hits)
    assert np.array_equal(got.token_sum, R * ref.token_sum) and np.array_equal(got.truth_count_sum, R * ref.truth_count_sum)
    assert got.accuracy(0) == ref.accuracy(0)


def test_out_of_domain_votes(hip_engine):
    from o1_inference_scaling_laws_amd.engine import Engine
    pool, _, tr = pool_of(4, 20, 21, 3, False)
    pool[1, 3], pool[2, 0] = -1, 4096
    tr[2] = 1023
    nv = np.array([1, 5, 20], dtype=np.int32)
    with pytest.raises(_lib.DomainError):
        hip_engine.resample_prefix(pool, tr, nv, 30, 1)
    dp, dtr, dnv = to_dev(pool, tr, nv)
    hip_engine.resample_prefix_device(dp, dtr, dnv, 0, 30, 1)
    with pytest.raises(_lib.DomainError):
        hip_engine.sync()
    want = resample.resample_prefix(pool, tr, nv, 0, 30, seed=1, M=21)
    assert want.error_bits & 1
    with Engine(device=0, clamp_to_invalid_bin=True) as ce:
        got = ce.resample_prefix(pool, tr, nv, 30, 1, M=21)
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.per_resample, want.per_resample)
        assert np.array_equal(got.truth_count_sum, want.truth_count_sum)


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(8, dtype=np.int32), (3, 1))                  # every subset is an all-way tie: n_modes == k
    tr = np.array([0, 1, 2], dtype=np.int32)
    nv = np.array([8], dtype=np.int32)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.resample_prefix(pool, tr, nv, 5, 1, M=8)
    assert ei.value.code == _lib.ERR_ARG
    dp, dtr, dnv = to_dev(pool, tr, nv)
    tie, _, _, _ = hip_engine.resample_prefix_device(dp, dtr, dnv, 0, 5, 1, M=4)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    assert int(tie.cpu().numpy()[0, 8]) == 15                               # the tie-class table itself is complete
    hip_engine.sync()                                                      # the word was cleared


def test_bad_shapes_are_refused_at_the_call(hip_engine):
    import ctypes as C
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 300), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nv = np.ones(40, dtype=np.int32)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, r0=0, r1=4, p_off=0, M=1, tok=None, tok_out=None, per=None, nvp=nv, tiep=tie):
        return L.scv_resample_prefix_i32(ctx, ptr(pool), ptr(tok), ptr(nvp), ptr(tr), 2, B, N, p_off, r0, r1, 1, M, _lib.MEM_HOST,
                                         ptr(tiep), ptr(tok_out), ptr(sums), ptr(per))
    assert call() == _lib.OK
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=33), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1),
               dict(tok_out=sums), dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(nvp=None), dict(tiep=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"resample" in L.scv_last_error(), kw
    _ = C


def test_first_call_of_a_fresh_context_and_a_captured_graph():
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    pool, tok, tr = pool_of(20, 128, 33, 1, True)
    nv = np.array([1 << k for k in range(8)], dtype=np.int32)
    want = resample.resample_prefix(pool, tr, nv, 0, 100, seed=4, tokens=tok, M=129)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    with Engine(device=0) as eng:                                          # no SCV_FLAG_TIMING: no event records in the graph
        got = eng.resample_prefix_device(dp, dtr, dnv, 0, 100, 4, tokens=dt, M=129)
        eng.sync()
        assert_same(got, want, True, 129)
        assert eng.stat("resample_calls") == 1
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got]
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
            eng.resample_prefix_device(dp, dtr, dnv, 0, 100, 4, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1],
                                       truth_count_sum=bufs[2], per_resample=bufs[3])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for b in bufs:
                b.zero_()
            eng.resample_prefix_device(dp, dtr, dnv, 0, 100, 4, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1],
                                       truth_count_sum=bufs[2], per_resample=bufs[3])
        for b in bufs:
            b.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eng.sync()
        assert_same(bufs, want, True, 129)


def test_the_reference_shape_through_the_engine_and_the_curve(hip_engine):
    P, N, R = 30, 128, 10_000
    pool, tok, tr = pool_of(P, N, 2025, 1, True)
    nv = np.array([1 << k for k in range(8)], dtype=np.int32)
    got = hip_engine.resample_prefix(pool, tr, nv, R, 17, tokens=tok, M=0)
    want = resample.resample_prefix(pool, tr, nv, 0, R, seed=17, tokens=tok)
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits)
    assert np.array_equal(got.token_sum, want.token_sum) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
    assert [got.accuracy(b) for b in range(8)] == [want.accuracy(b) for b in range(8)]
    limits = [2 ** i for i in range(11, 19)]
    recs = curves.expected_majority_records(hip_engine, pool, tr, tok, limits, R, 17)
    assert [r["token_limit"] for r in recs] == limits
    assert [r["accuracy"] for r in recs] == [got.accuracy(b) for b in range(8)]
    assert [r["avg_tokens_used"] for r in recs] == [float(got.avg_tokens_used(b)) for b in range(8)]
