"""GPU tests of scv_iid_prefix_i32 (majority vote over draws with replacement, past the size of the pool): every output bit-exact against
the CPU mirror (o1_inference_scaling_laws_amd/iid.py), identities that need no mirror, DEVICE against HOST (one chunk and two), slices and
shards, forced grids, a captured graph, and the errors."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, curves, iid, synth

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 8, 63, 64, 65, 128, 129, 255, 256]
RS = [1, 3, 64, 65, 1000]
BS = [1, 8, 32]


def budget_choices(N):
    return [-3, 0, 1, N - 1, N, N + 1, 2 * N, 255, 256, 257, 1000]


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


def assert_result(got, want, tokens=True, per=True):
    assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
    if tokens:
        assert np.array_equal(got.token_sum, want.token_sum)
    if per:
        assert np.array_equal(got.per_resample, want.per_resample)


@pytest.fixture
def grid_option(hip_engine):
    try:
        yield lambda g: hip_engine.set_option("grid", g)
    finally:
        hip_engine.set_option("grid", 0)


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N, tokens):
    eng = hip_engine
    for dist in range(6):
        k = 6 * NS.index(N) + dist + (3 if tokens else 0)
        R = RS[k % len(RS)]
        P = 2 if R >= 1000 else (3, 5)[k % 2]                              # P * R: 2000 or an odd multiple of R, never whole workgroups
        B = BS[(k // 2) % 3]
        rng = np.random.default_rng(900 + k)
        nd = rng.choice(budget_choices(N), size=B).astype(np.int32)
        if dist == 0:
            nd[0] = 1000
        r0 = (0, 7, 2 ** 31 - 1 - R)[k % 3]
        p_off = (0, 5, 1 << 33)[(k + 1) % 3]
        M = (N + 1) if k % 2 == 0 else 0
        pool, tok, tr = pool_of(P, N, 60 + k, dist, tokens)
        want = iid.iid_prefix(pool, tr, nd, r0, r0 + R, 3000 + k, tokens=tok, p_offset=p_off, M=M)
        dp, dt, dtr, dnd = to_dev(pool, tok, tr, nd)
        got = eng.iid_prefix_device(dp, dtr, dnd, r0, r0 + R, 3000 + k, tokens=dt, p_offset=p_off, M=M if M else None)
        eng.sync()
        assert want.error_bits == 0
        assert_same(got, want, tokens, M)


@pytest.mark.parametrize("k,P,R", [(4096, 3, 65), (65535, 2, 3)])
def test_long_walks_are_bit_exact(hip_engine, k, P, R):
    pool, tok, tr = pool_of(P, 128, 5 + k, 1, True)
    nd = np.array([k, 129, k - 1, 1], dtype=np.int32)
    want = iid.iid_prefix(pool, tr, nd, 2, 2 + R, 99, tokens=tok, M=129)
    got = hip_engine.iid_prefix(pool, tr, nd, R, 99, tokens=tok, r_begin=2, M=129)
    assert_result(got, want)
    assert int(want.token_sum[0]) > int(want.token_sum[1]) > 0


def test_identities_that_need_no_mirror(hip_engine):
    eng = hip_engine
    R = 37
    nd = np.array([1, 2, 7, 300, 0, 1000], dtype=np.int32)
    for dist, N in ((2, 40), (5, 40), (1, 1), (3, 1)):                     # one repeated value per pool: D2 (the truth), D5 (a wrong one); N = 1
        pool, _, tr = pool_of(11, N, 8 + dist, dist, False)
        assert (pool == pool[:, :1]).all()
        hits = int((pool[:, 0] == tr).sum())
        assert hits == {2: 11, 5: 0}.get(dist, hits)
        got = eng.iid_prefix(pool, tr, nd, R, 4, M=0)
        for b, kb in enumerate(nd.tolist()):
            want = np.zeros(1025, dtype=np.int64)
            if kb >= 1:
                want[1] = hits * R                                          # every draw is that value: a unique mode for every k >= 1
            assert np.array_equal(got.tie_class_hits[b], want), (dist, N, kb)
            assert got.truth_count_sum[b] == hits * R * kb
    pool, tok, tr = pool_of(9, 77, 3, 1, True)                             # k = 1: the cell hits exactly when its one draw is the truth
    got = eng.iid_prefix(pool, tr, np.array([1, 1, 5], dtype=np.int32), 500, 6, tokens=tok, M=0)
    assert got.tie_class_hits[0, 1] == got.truth_count_sum[0] > 0 and got.tie_class_hits[0].sum() == got.tie_class_hits[0, 1]
    assert np.array_equal(got.tie_class_hits[0], got.tie_class_hits[1]) and got.token_sum[0] == got.token_sum[1]


def test_device_equals_host_and_host_overwrites(hip_engine):
    eng = hip_engine
    pool, tok, tr = pool_of(9, 40, 3, 1, True)
    nd = np.array([1, 2, 40, 41, 100, 300, 7], dtype=np.int32)
    want = iid.iid_prefix(pool, tr, nd, 0, 70, 5, tokens=tok, M=41)
    for _ in range(2):                                                     # HOST: the same answer twice, not twice the answer
        got = eng.iid_prefix(pool, tr, nd, 70, 5, tokens=tok, M=41)
        assert_result(got, want)
        assert got.accuracy(4) == want.accuracy(4) and got.exact_accuracy(5) == want.exact_accuracy(5)
    assert eng.iid_prefix(pool, tr, nd, 70, 5, tokens=tok).per_resample.shape == (70, 7, 41)      # M None: min(max budget, N) + 1
    dp, dt, dtr, dnd = to_dev(pool, tok, tr, nd)
    bufs = eng.iid_prefix_device(dp, dtr, dnd, 0, 70, 5, tokens=dt, M=41)
    eng.iid_prefix_device(dp, dtr, dnd, 0, 70, 5, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2], per_resample=bufs[3])
    eng.sync()
    for b, w in zip(bufs, (want.tie_class_hits, want.token_sum, want.truth_count_sum, want.per_resample)):
        assert np.array_equal(b.cpu().numpy(), 2 * w)                      # DEVICE accumulates


def test_two_chunk_host_call_equals_the_device_call(hip_engine):
    """P = 70 000 rows of 256 votes are 68 MiB of pool: the HOST call stages two chunks (64 MiB each at most), each with its p_offset."""
    eng = hip_engine
    P, N = 70_000, 256
    rng = np.random.default_rng(12)
    pool = rng.integers(0, 5, size=(P, N), dtype=np.int32)
    tr = rng.integers(0, 5, size=P).astype(np.int32)
    nd = np.array([8, 1, 3, 0], dtype=np.int32)
    host = eng.iid_prefix(pool, tr, nd, 1, 21, r_begin=4, p_offset=10, M=9)
    dp, dtr, dnd = to_dev(pool, tr, nd)
    dev = eng.iid_prefix_device(dp, dtr, dnd, 4, 5, 21, p_offset=10, M=9)
    eng.sync()
    assert np.array_equal(dev[0].cpu().numpy(), host.tie_class_hits) and np.array_equal(dev[2].cpu().numpy(), host.truth_count_sum)
    assert np.array_equal(dev[3].cpu().numpy(), host.per_resample)
    assert host.tie_class_hits[1, 1] == host.truth_count_sum[1] and 0 < host.tie_class_hits[0].sum() < P and not host.tie_class_hits[3].any()
    tail = slice(69_990, P)                                                # the last problems lie in the second chunk: against the mirror
    want = iid.iid_prefix(pool[tail], tr[tail], nd, 4, 5, 21, p_offset=10 + 69_990, M=9)
    part = eng.iid_prefix(pool[tail], tr[tail], nd, 1, 21, r_begin=4, p_offset=10 + 69_990, M=9)
    assert_result(part, want, tokens=False)


def test_slices_and_shards_add_up_on_the_device(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 100, 9, 4, True)
    nd = np.array([100, 1, 264, 7, 32], dtype=np.int32)
    want = iid.iid_prefix(pool, tr, nd, 3, 203, 11, tokens=tok, M=101)
    dp, dt, dtr, dnd = to_dev(pool, tok, tr, nd)
    tie, ts, tcs, _ = eng.iid_prefix_device(dp, dtr, dnd, 3, 80, 11, tokens=dt)
    eng.iid_prefix_device(dp, dtr, dnd, 80, 203, 11, tokens=dt, tie_class_hits=tie, token_sum=ts, truth_count_sum=tcs)
    per = torch.zeros((200, 5, 101), dtype=torch.int64, device=dp.device)
    for lo, hi in ((0, 4), (4, 11)):                                       # problem shards, each with its global offset
        eng.iid_prefix_device(dp[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dnd, 3, 203, 11, tokens=dt[lo:hi].contiguous(),
                              p_offset=lo, per_resample=per)
    eng.sync()
    assert np.array_equal(tie.cpu().numpy(), want.tie_class_hits)
    assert np.array_equal(ts.cpu().numpy(), want.token_sum) and np.array_equal(tcs.cpu().numpy(), want.truth_count_sum)
    assert np.array_equal(per.cpu().numpy(), want.per_resample)


@pytest.mark.parametrize("grid", [1, 3])
def test_forced_grids(hip_engine, grid_option, grid):
    pool, tok, tr = pool_of(7, 65, 2, 3, True)
    nd = np.array([1, 64, 65, 66, 130, 400], dtype=np.int32)
    want = iid.iid_prefix(pool, tr, nd, 0, 300, 8, tokens=tok, M=66)
    grid_option(grid)
    assert_result(hip_engine.iid_prefix(pool, tr, nd, 300, 8, tokens=tok, M=66), want)


def test_a_captured_graph_replayed_twice_accumulates_twice():
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    pool, tok, tr = pool_of(20, 128, 33, 1, True)
    nd = np.array([1, 16, 128, 200, 512], dtype=np.int32)
    want = iid.iid_prefix(pool, tr, nd, 0, 100, 4, tokens=tok, M=129)
    dp, dt, dtr, dnd = to_dev(pool, tok, tr, nd)
    with Engine(device=0) as eng:                                          # no SCV_FLAG_TIMING: no event records in the graph
        got = eng.iid_prefix_device(dp, dtr, dnd, 0, 100, 4, tokens=dt, M=129)     # the first call of a fresh context
        eng.sync()
        assert_same(got, want, True, 129)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got]
        kw = dict(tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2], per_resample=bufs[3])
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
            eng.iid_prefix_device(dp, dtr, dnd, 0, 100, 4, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.iid_prefix_device(dp, dtr, dnd, 0, 100, 4, **kw)
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        eng.sync()
        for b, w in zip(bufs, (want.tie_class_hits, want.token_sum, want.truth_count_sum, want.per_resample)):
            assert np.array_equal(b.cpu().numpy(), 2 * w)


def test_bad_arguments_are_refused_at_the_call(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 300), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nd = np.ones(40, dtype=np.int32)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, r0=0, r1=4, p_off=0, M=1, tok=None, tok_out=None, per=None, ndp=nd, tiep=tie):
        return L.scv_iid_prefix_i32(ctx, ptr(pool), ptr(tok), ptr(ndp), ptr(tr), 2, B, N, p_off, r0, r1, 1, M, _lib.MEM_HOST,
                                    ptr(tiep), ptr(tok_out), ptr(sums), ptr(per))
    assert call() == _lib.OK
    big = nd.copy()
    big[1] = _lib.IID_MAX_DRAWS + 1
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=33), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1),
               dict(tok_out=sums), dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(ndp=None), dict(tiep=None), dict(ndp=big)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"iid" in L.scv_last_error(), kw
    big[1] = _lib.IID_MAX_DRAWS                                             # the limit itself is legal; B = 1 does not read big[1]
    assert call(ndp=big, B=1) == _lib.OK


def test_a_budget_above_the_limit_in_device_mode(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(5, 16, 1, 1, True)
    nd = np.array([4, 65536, 2], dtype=np.int32)
    dp, dt, dtr, dnd = to_dev(pool, tok, tr, nd)
    bufs = [torch.full(s, 7, dtype=torch.int64, device=dp.device) for s in ((3, 1025), (3,), (3,), (10, 3, 17))]
    eng.iid_prefix_device(dp, dtr, dnd, 0, 10, 1, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2], per_resample=bufs[3])
    word = torch.zeros(1, dtype=torch.int64, device=dp.device)
    eng.export_error_word(word)
    with pytest.raises(_lib.ScvError) as ei:
        eng.sync()
    assert ei.value.code == _lib.ERR_ARG and "SCV_IID_MAX_DRAWS" in str(ei.value)
    assert int(word.item()) == _lib.ERR_BIT_IID_DRAWS == iid.ERR_DRAWS_BIT == 128
    assert all(bool((b == 7).all()) for b in bufs)                          # nothing was computed
    eng.sync()                                                             # the word was cleared
    want = iid.iid_prefix(pool, tr, nd, 0, 10, 1, tokens=tok, M=17)
    assert want.error_bits == 128 and not want.tie_class_hits.any()


def test_out_of_domain_votes(hip_engine):
    from o1_inference_scaling_laws_amd.engine import Engine
    pool, _, tr = pool_of(4, 20, 21, 3, False)
    pool[1, 3], pool[2, 0] = -1, 4096
    tr[2] = 1023
    nd = np.array([1, 5, 20, 90], dtype=np.int32)
    with pytest.raises(_lib.DomainError):
        hip_engine.iid_prefix(pool, tr, nd, 30, 1)
    dp, dtr, dnd = to_dev(pool, tr, nd)
    hip_engine.iid_prefix_device(dp, dtr, dnd, 0, 30, 1)
    with pytest.raises(_lib.DomainError):
        hip_engine.sync()
    want = iid.iid_prefix(pool, tr, nd, 0, 30, 1, M=21)
    assert want.error_bits & 1
    with Engine(device=0, clamp_to_invalid_bin=True) as ce:
        assert_result(ce.iid_prefix(pool, tr, nd, 30, 1, M=21), want, tokens=False)


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(2, dtype=np.int32), (3, 1))                  # two values, two draws: a two-way tie half of the time
    tr = np.array([0, 1, 0], dtype=np.int32)
    nd = np.array([2], dtype=np.int32)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.iid_prefix(pool, tr, nd, 64, 1, M=2)
    assert ei.value.code == _lib.ERR_ARG
    dp, dtr, dnd = to_dev(pool, tr, nd)
    tie, _, _, _ = hip_engine.iid_prefix_device(dp, dtr, dnd, 0, 64, 1, M=2)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    want = iid.iid_prefix(pool, tr, nd, 0, 64, 1, M=2)
    assert want.error_bits == 2 and want.tie_class_hits[0, 2] > 0
    assert np.array_equal(tie.cpu().numpy(), want.tie_class_hits)          # the tie-class table itself is complete
    hip_engine.sync()                                                      # the word was cleared


def test_the_curve_goes_past_the_pool_and_ends_in_its_limit(hip_engine):
    pool, tok, tr = pool_of(30, 128, 2025, 1, True)
    draws = [1, 8, 128, 1024]
    recs = curves.iid_majority_records(hip_engine, pool, tr, tok, draws, 200, 17)
    want = iid.iid_prefix(pool, tr, np.array(draws), 0, 200, 17, tokens=tok)
    assert [r["samples"] for r in recs] == draws + [float("inf")]
    assert [r["accuracy"] for r in recs[:-1]] == [want.accuracy(b) for b in range(4)]
    assert [r["avg_tokens_used"] for r in recs[:-1]] == [float(want.avg_tokens_used(b)) for b in range(4)]
    assert recs[-1]["accuracy"] == hip_engine.aggregate_prefix(pool, tr, np.array([128], dtype=np.int32), want_cells=False).accuracy(0)
