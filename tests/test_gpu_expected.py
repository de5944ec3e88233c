"""GPU tests of scv_expected_majority_i32 (exact expected majority vote over all k-subsets of a pool): every output within 1e-12 relative
of the rational mirror (o1_inference_scaling_laws_amd/expected.py) and exactly 0.0 where it is 0, the k = 1, 2, N identities, bit-identity
across HOST / DEVICE / repeats / shards, a fresh context, a captured graph, errors, and agreement with the sampled estimator."""
import math

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, expected, resample, synth
from o1_inference_scaling_laws_amd.engine import Engine

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 8, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200, 255, 256]


def budgets_for(N, variant):
    ref = [1 << k for k in range(N.bit_length()) if (1 << k) <= N]
    if variant == 0:
        return ref
    if variant == 1:
        return ref[::-1] + [N, 0, N + 5]
    rng = np.random.default_rng(N)
    return rng.integers(-2, N + 3, size=32).tolist()


def pool_of(P, N, seed, dist):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    return a[:, 0, :].copy(), t[:, 0, :].copy(), tr


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def assert_close(got, want):
    for p, row in enumerate(want):
        for b, r in enumerate(row):
            g = float(got[p, b])
            if r == 0:
                assert g == 0.0, (p, b, g)
            else:
                assert abs(g - float(r)) <= 1e-12 * float(r), (p, b, g, float(r))


@pytest.mark.parametrize("N", NS)
def test_against_the_rational_mirror(hip_engine, N):
    eng = hip_engine
    for dist in range(6):
        k = NS.index(N) + dist
        nv = np.array(budgets_for(N, k % 3), dtype=np.int32)
        pool, _tok, tr = pool_of(3, N, 70 + k, dist)
        if k % 4 == 1:
            tr[0] = 5000                                                    # a truth outside the bins never hits
        E, H = expected.expected_majority_exact(pool, tr, nv)
        dp, dtr, dnv = to_dev(pool, tr, nv)
        score, hit = eng.expected_majority_device(dp, dtr, dnv)
        eng.sync()
        assert_close(score.cpu().numpy(), E)
        assert_close(hit.cpu().numpy(), H)


def test_small_budgets_and_the_whole_pool(hip_engine):
    eng = hip_engine
    for dist in range(6):
        N = 40 + 7 * dist
        pool, _tok, tr = pool_of(8, N, 11 + dist, dist)
        res = eng.expected_majority(pool, tr, np.array([1, 2, N], dtype=np.int32))
        ct = (pool == tr[:, None]).sum(axis=1)
        assert np.allclose(res.score[:, 0], ct / N, rtol=1e-12, atol=0) and np.allclose(res.score[:, 1], ct / N, rtol=1e-12, atol=0)
        assert np.allclose(res.hit_prob[:, 0], ct / N, rtol=1e-12, atol=0)
        for p in range(8):                                                   # k = N: the whole-pool score of scv_aggregate_prefix_i32
            out = eng.aggregate_prefix(pool[p:p + 1], tr[p:p + 1], np.array([N], dtype=np.int32), want_cells=False)
            tie = out.tie_class_hits[0]
            whole = sum(tie[m] / m for m in range(1, _lib.TIE_CLASSES) if tie[m])
            assert abs(res.score[p, 2] - whole) <= 1e-12 * max(whole, 1e-300), (p, res.score[p, 2], whole)


def test_host_device_repeats_and_shards_are_bit_identical(hip_engine):
    eng = hip_engine
    pool, _tok, tr = pool_of(37, 128, 5, 1)
    nv = np.array(budgets_for(128, 2), dtype=np.int32)
    a = eng.expected_majority(pool, tr, nv)
    b = eng.expected_majority(pool, tr, nv)
    assert np.array_equal(a.score, b.score) and np.array_equal(a.hit_prob, b.hit_prob)
    dp, dtr, dnv = to_dev(pool, tr, nv)
    s, h = eng.expected_majority_device(dp, dtr, dnv)
    s2, h2 = eng.expected_majority_device(dp, dtr, dnv, score=s, hit_prob=h)         # overwrite, not accumulate
    eng.sync()
    assert np.array_equal(s2.cpu().numpy(), a.score) and np.array_equal(h2.cpu().numpy(), a.hit_prob)
    for p0, p1 in ((0, 1), (1, 20), (20, 37)):
        part = eng.expected_majority(pool[p0:p1], tr[p0:p1], nv)
        assert np.array_equal(part.score, a.score[p0:p1]) and np.array_equal(part.hit_prob, a.hit_prob[p0:p1])
    no_hit = eng.expected_majority(pool, tr, nv, hit_prob=False)
    assert no_hit.hit_prob is None and np.array_equal(no_hit.score, a.score)


def test_fresh_context_and_graph_capture():
    import torch
    pool, _tok, tr = pool_of(9, 64, 8, 2)
    nv = np.array([1, 3, 8, 64, 0], dtype=np.int32)
    E, H = expected.expected_majority_exact(pool, tr, nv)
    with Engine() as eng:                                                    # the first call of a fresh context
        res = eng.expected_majority(pool, tr, nv)
        assert_close(res.score, E)
        assert_close(res.hit_prob, H)
        dp, dtr, dnv = to_dev(pool, tr, nv)
        score = torch.zeros((9, 5), dtype=torch.float64, device="cuda")
        hit = torch.zeros((9, 5), dtype=torch.float64, device="cuda")
        eng.expected_majority_device(dp, dtr, dnv, score=score, hit_prob=hit)     # warm-up outside the capture
        torch.cuda.synchronize()
        score.zero_()
        hit.zero_()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                eng.expected_majority_device(dp, dtr, dnv, score=score, hit_prob=hit)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(score.cpu().numpy(), res.score) and np.array_equal(hit.cpu().numpy(), res.hit_prob)


def test_errors_domain_and_stat(hip_engine):
    eng = hip_engine
    L = _lib.load()
    pool, _tok, tr = pool_of(4, 16, 3, 0)
    nv = np.array([1, 4, 16], dtype=np.int32)
    for P, B, N in ((4, 3, 0), (4, 3, 257), (4, 0, 16), (4, 33, 16), (-1, 3, 16)):
        out = np.zeros((max(P, 1), max(B, 1)))
        assert L.scv_expected_majority_i32(eng._ctx, pool.ctypes.data, nv.ctypes.data, tr.ctypes.data, P, B, N, _lib.MEM_HOST,
                                           out.ctypes.data, None) == _lib.ERR_ARG
    out = np.zeros((4, 3))
    assert L.scv_expected_majority_i32(eng._ctx, pool.ctypes.data, nv.ctypes.data, tr.ctypes.data, 4, 3, 16, _lib.MEM_HOST, None, None) == _lib.ERR_ARG
    assert L.scv_expected_majority_i32(eng._ctx, None, nv.ctypes.data, tr.ctypes.data, 4, 3, 16, _lib.MEM_HOST, out.ctypes.data, None) == _lib.ERR_ARG
    assert L.scv_expected_majority_i32(eng._ctx, pool.ctypes.data, None, tr.ctypes.data, 4, 3, 16, _lib.MEM_HOST, out.ctypes.data, None) == _lib.ERR_ARG
    assert L.scv_expected_majority_i32(eng._ctx, None, nv.ctypes.data, None, 0, 3, 16, _lib.MEM_HOST, out.ctypes.data, None) == _lib.OK
    before = eng.stat("expected_calls")
    eng.expected_majority(pool, tr, nv)
    assert eng.stat("expected_calls") == before + 1
    bad = pool.copy()
    bad[1, 3] = -7                                                           # counts as value 1023
    with pytest.raises(_lib.ScvError):
        eng.expected_majority(bad, tr, nv)
    dp, dtr, dnv = to_dev(bad, tr, nv)
    eng.expected_majority_device(dp, dtr, dnv)
    with pytest.raises(_lib.ScvError):
        eng.sync()
    with Engine(clamp_to_invalid_bin=True) as clamped:
        res = clamped.expected_majority(bad, tr, nv)
        E, H = expected.expected_majority_exact(bad, tr, nv)
        assert_close(res.score, E)
        assert_close(res.hit_prob, H)


def test_agrees_with_the_sampled_estimator(hip_engine):
    eng = hip_engine
    P, N, R = 30, 128, 4096
    pool, _tok, tr = pool_of(P, N, 2024, 1)
    nv = np.array([1, 2, 4, 8, 16, 32, 64, 128], dtype=np.int32)
    ex = eng.expected_majority(pool, tr, nv)
    rs = eng.resample_prefix(pool, tr, nv, R, seed=7, M=0)
    for b in range(len(nv)):
        assert abs(rs.accuracy(b) - ex.accuracy(b)) <= 3 / math.sqrt(P * R), (b, rs.accuracy(b), ex.accuracy(b))


def test_the_reference_shape_through_curves(hip_engine):
    from o1_inference_scaling_laws_amd import curves
    pool, tok, tr = pool_of(30, 128, 9, 1)
    recs = curves.exact_majority_records(hip_engine, pool, tr, tok, [2 ** 11 * n for n in (1, 2, 4, 8, 16, 32, 64, 128)])
    E, _H = expected.expected_majority_exact(pool, tr, [1, 2, 4, 8, 16, 32, 64, 128])
    for b, r in enumerate(recs):
        want = float(sum(E[p][b] for p in range(30)) / 30)
        assert abs(r["accuracy"] - want) <= 1e-12 * max(want, 1e-300)
    assert recs[-1]["avg_tokens_used"] == float(int(tok.astype(np.int64).sum())) / 30
    assert resample.MAX_N == expected.MAX_N
