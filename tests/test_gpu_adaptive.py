"""GPU tests of scv_adaptive_prefix_i32 (the majority vote that samples until a stopping rule says it is settled): every output bit-exact
against the CPU mirror (o1_inference_scaling_laws_amd/adaptive.py) in both orders, the reductions to the live scv_resample_prefix_i32 /
scv_aggregate_prefix_i32 under `never`, edges (caps of 0 and beyond N, 32 identical rules, 256 equal or distinct votes, grids, a two-chunk
HOST call, more than 2^32 stops through one workgroup's tie and stop tables), HOST against DEVICE, slices and shards, a captured graph, the
clamp flag and the errors."""
import time

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, adaptive, curves, synth
from o1_inference_scaling_laws_amd.adaptive import STOP_DECIDED, beta_rule, margin_rule, never
from o1_inference_scaling_laws_amd.engine import TIE_CLASSES, Engine, cells_from_torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 8, 16, 63, 64, 65, 127, 128, 129, 200, 255, 256]
RS = [1, 3, 64, 65, 300]
BS = [1, 8, 32]
FIELDS = ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "stop_hist")


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


def rules_for(N, B, seed):
    """ragged caps (negative, 0, inside, N, beyond N), random need tables (values below 0 and above N + 1 too), built rules, both flags."""
    rng = np.random.default_rng(seed)
    cap = rng.choice([-3, 0, 1, max(1, N // 2), N, N + 7] + rng.integers(0, N + 1, size=4).tolist(), size=B).astype(np.int32)
    need = rng.integers(-2, N + 4, size=(B, N + 1)).astype(np.int32)
    built = [never(N), margin_rule(N, 1), margin_rule(N, 2), margin_rule(N, 3), beta_rule(N, 0.9), beta_rule(N, 0.95)]
    for b in range(B):
        if rng.random() < 0.6:
            need[b] = built[int(rng.integers(len(built)))]
    flags = rng.integers(0, 2, size=B).astype(np.int32)
    return cap, need, flags


def assert_same(got, want, M, cells=False):
    """got: the tuple of adaptive_prefix_device; want: an AdaptiveResult."""
    tie, ts, vs, tcs, hist, per, c, ct, cv = [None if x is None else x.cpu().numpy() for x in got]
    assert np.array_equal(tie, want.tie_class_hits) and np.array_equal(hist, want.stop_hist)
    assert np.array_equal(vs, want.vote_count_sum) and np.array_equal(tcs, want.truth_count_sum)
    assert (ts is None and want.token_sum is None) or np.array_equal(ts, want.token_sum)
    if M:
        assert np.array_equal(per, want.per_resample)
    if cells:
        assert np.array_equal(cells_from_torch(got[6]), want.cells) and np.array_equal(cv, want.cell_votes)
        assert (ct is None and want.cell_tokens is None) or np.array_equal(ct, want.cell_tokens)


def assert_host_same(got, want, M, cells=False):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None and b is None) or np.array_equal(a, b), f
    if M:
        assert np.array_equal(got.per_resample, want.per_resample)
    if cells:
        assert np.array_equal(got.cells, want.cells) and np.array_equal(got.cell_votes, want.cell_votes)
        assert (got.cell_tokens is None and want.cell_tokens is None) or np.array_equal(got.cell_tokens, want.cell_tokens)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N, shuffled):
    eng = hip_engine
    for dist in range(6):
        k = NS.index(N) + dist
        B = BS[k % 3]
        R = RS[k % len(RS)] if shuffled else 1
        P = (2 if R >= 300 else 3 + k % 3) if shuffled else 5 + 7 * (k % 4)
        r0 = (0, 7, 2 ** 31 - 1 - R)[k % 3] if shuffled else 0
        p_off = (0, 5, 1 << 33)[(k + 1) % 3] if shuffled else 0
        seed = 2024 + k
        pool, tok, tr = pool_of(P, N, 40 + k, dist)
        cap, need, flags = rules_for(N, B, k)
        use_tok = k % 4 != 0
        fl = flags if k % 5 else None                                   # NULL rule_flags: all 0
        M = N + 1
        want = adaptive.adaptive_prefix(pool, tr, cap, need, fl, tokens=tok if use_tok else None, r_begin=r0,
                                        r_end=r0 + R if shuffled else None, seed=seed, p_offset=p_off, M=M, want_cells=not shuffled)
        assert want.error_bits == 0
        dp, dt, dtr, dc, dn, df = to_dev(pool, tok if use_tok else None, tr, cap, need, fl)
        got = eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=r0, r_end=r0 + R if shuffled else None, seed=seed,
                                         p_offset=p_off, M=M, want_cells=not shuffled)
        eng.sync()
        assert_same(got, want, M, cells=not shuffled)
        host = eng.adaptive_prefix(pool, tr, cap, need, fl, tokens=tok if use_tok else None, resamples=R if shuffled else None, seed=seed,
                                   r_begin=r0, p_offset=p_off, M=M, want_cells=not shuffled)
        assert_host_same(host, want, M, cells=not shuffled)
        assert (host.stop_hist.sum(axis=1) == P * R).all()
        assert np.array_equal((host.stop_hist * np.arange(N + 1)).sum(axis=1), host.vote_count_sum)


@pytest.mark.parametrize("N", [1, 8, 64, 65, 128, 256])
def test_never_matches_the_live_resample_and_prefix_kernels(hip_engine, N):
    """`never` with flag 0 == scv_resample_prefix_i32 at k = cap (tie, token, truth, per_resample; stop_hist a spike at n_max); with
    SCV_STOP_DECIDED the same tie classes and per_resample at no more votes; in pool order its cells are scv_aggregate_prefix_i32's."""
    import torch
    eng = hip_engine
    P, R = 24, 33
    rng = np.random.default_rng(N)
    cap = np.concatenate([[0, 1, N, N + 3, -1], rng.integers(0, N + 1, size=5)]).astype(np.int32)
    B = len(cap)
    nmax = np.clip(cap, 0, N).astype(np.int64)
    need = np.tile(never(N), (B, 1))
    dec_flags = np.full(B, STOP_DECIDED, dtype=np.int32)
    for dist in range(6):
        pool, tok, tr = pool_of(P, N, 10 * N + dist, dist)
        dp, dt, dtr, dc, dn, df = to_dev(pool, tok, tr, cap, need, dec_flags)
        got = eng.adaptive_prefix_device(dp, dtr, dc, dn, None, tokens=dt, r_begin=9, r_end=9 + R, seed=3, p_offset=4, M=N + 1)
        ref = eng.resample_prefix_device(dp, dtr, dc, 9, 9 + R, 3, tokens=dt, p_offset=4, M=N + 1)
        dec = eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=9, r_end=9 + R, seed=3, p_offset=4, M=N + 1)
        eng.sync()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[2]) and torch.equal(got[5], ref[3])
        hist = got[4].cpu().numpy()
        for b in range(B):
            spike = np.zeros(N + 1, dtype=np.int64)
            spike[nmax[b]] = P * R
            assert np.array_equal(hist[b], spike)
        assert np.array_equal(got[2].cpu().numpy(), nmax * P * R)
        assert torch.equal(dec[0], got[0]) and torch.equal(dec[5], got[5])
        assert bool((dec[2] <= got[2]).all()) and bool((dec[1] <= got[1]).all())
        if dist == 2:                                                   # every vote the same: decided after n_max // 2 + 1 samples
            assert np.array_equal(dec[2].cpu().numpy(), np.where(nmax > 0, nmax // 2 + 1, 0) * P * R)
            assert N == 1 or int(dec[2][2]) < int(got[2][2])
        pcell = eng.adaptive_prefix_device(dp, dtr, dc, dn, None, tokens=dt, want_cells=True)
        counters, rcells, rct = eng.aggregate_prefix_device(dp, dtr, to_dev(nmax.astype(np.int32))[0], tokens=dt)
        eng.sync()
        assert np.array_equal(cells_from_torch(pcell[6]), cells_from_torch(rcells)) and torch.equal(pcell[7], rct)
        assert np.array_equal(pcell[8].cpu().numpy(), np.tile(nmax.astype(np.int32), (P, 1)))
        cnt = counters.cpu().numpy()
        assert np.array_equal(pcell[0].cpu().numpy().reshape(-1), cnt[: B * TIE_CLASSES])
        assert np.array_equal(pcell[1].cpu().numpy(), cnt[B * TIE_CLASSES: B * TIE_CLASSES + B])
        assert np.array_equal(pcell[3].cpu().numpy(), cnt[B * TIE_CLASSES + B:])


def test_caps_of_zero_and_beyond_n(hip_engine):
    pool, tok, tr = pool_of(7, 50, 5, 2)                                # every vote the truth: any non-empty cell hits
    cap = np.array([0, -5, 0, 500, 50], dtype=np.int32)
    for R in (None, 70):
        got = hip_engine.adaptive_prefix(pool, tr, cap, margin_rule(50, 3), tokens=tok, resamples=R, seed=1, want_cells=R is None)
        cells = 7 * (R or 1)
        assert not got.tie_class_hits[:3].any() and not got.token_sum[:3].any() and not got.vote_count_sum[:3].any()
        assert (got.stop_hist[:3, 0] == cells).all() and not got.stop_hist[:3, 1:].any() and not got.per_resample[:, :3].any()
        assert (got.tie_class_hits[3:, 1] == cells).all() and (got.stop_hist[3:, 3] == cells).all()      # 3 equal votes: a lead of 3
        if R is None:
            assert (got.cells["max_count"][:, :3] == 0).all() and (got.cells["min_mode"][:, :3] == -1).all()
            assert not got.cell_tokens[:, :3].any() and not got.cell_votes[:, :3].any() and (got.cell_votes[:, 3:] == 3).all()


@pytest.mark.parametrize("shuffled", [False, True])
def test_256_equal_and_256_distinct_votes(hip_engine, shuffled):
    rng = np.random.default_rng(256)
    pool = np.stack([np.full(256, 17), rng.permutation(1024)[:256], np.full(256, 17), rng.permutation(1024)[:256]]).astype(np.int32)
    tr = np.array([17, int(pool[1, 5]), 18, 2000], dtype=np.int32)
    tok = rng.integers(0, 5000, size=pool.shape).astype(np.int32)
    cap = np.array([256, 256, 256, 1000, 100], dtype=np.int32)
    need = np.stack([never(256), never(256), margin_rule(256, 200), beta_rule(256, 0.99), margin_rule(256, 2)])
    flags = np.array([0, STOP_DECIDED, 0, 0, STOP_DECIDED], dtype=np.int32)
    R = 16 if shuffled else None
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=R, seed=9, M=257, want_cells=not shuffled)
    got = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=R, seed=9, M=257, want_cells=not shuffled)
    assert_host_same(got, want, 257, cells=not shuffled)
    r = R or 1
    assert got.tie_class_hits[0, 1] == r and got.tie_class_hits[0, 256] == r and got.tie_class_hits[0].sum() == 2 * r
    assert got.vote_count_sum[0] == 4 * 256 * r and got.vote_count_sum[1] == (2 * 129 + 2 * 256) * r


def test_32_identical_rules(hip_engine):
    pool, tok, tr = pool_of(20, 128, 3, 1)
    cap = np.full(32, 128, dtype=np.int32)
    need = np.tile(beta_rule(128, 0.95), (32, 1))
    flags = np.full(32, STOP_DECIDED, dtype=np.int32)
    got = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=100, seed=2)
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=100, seed=2, M=129)
    assert_host_same(got, want, 129)
    assert (got.tie_class_hits == got.tie_class_hits[0]).all() and (got.token_sum == got.token_sum[0]).all()
    assert (got.stop_hist == got.stop_hist[0]).all() and 0 < got.vote_count_sum[0] < 128 * 20 * 100


def test_32_rules_at_n_256_fit_the_lds(hip_engine):
    """B = 32, N = 256: the tie, stop and need tables alone are about 82 KB of the workgroup's LDS."""
    pool, tok, tr = pool_of(6, 256, 8, 0)
    cap, need, flags = rules_for(256, 32, 4)
    for R in (None, 40):
        want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=R, seed=6, M=257, want_cells=R is None)
        got = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=R, seed=6, M=257, want_cells=R is None)
        assert_host_same(got, want, 257, cells=R is None)


def test_grid_option_keeps_the_bits(hip_engine, grid_option):
    pool, tok, tr = pool_of(12, 256, 12, 3)
    cap, need, flags = rules_for(256, 8, 12)
    ref_s = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=64, seed=3, r_begin=5)
    ref_p = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True)
    assert_host_same(ref_s, adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_begin=5, r_end=69, seed=3, M=257), 257)
    for g in (1, 3):
        grid_option(g)
        assert_host_same(hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=64, seed=3, r_begin=5), ref_s, True)
        assert_host_same(hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True), ref_p, True, cells=True)


def test_host_staging_chunks_match_one_device_launch(hip_engine):
    P, N = 30_000, 256                 # pool order with every cell output: 64 MiB / (2 * 256 * 4 + 4 + 32 * (16 + 8 + 4)) = 22 764 pools per chunk
    a, t, tr = synth.fill(P, 1, N, 31, 1, want_tokens=True)
    pool, tok = np.ascontiguousarray(a[:, 0, :]), np.ascontiguousarray(t[:, 0, :])
    cap, need, flags = rules_for(N, 32, 31)
    host = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True)
    dev = hip_engine.adaptive_prefix_device(*to_dev(pool, tr, cap, need, flags), tokens=to_dev(tok)[0], want_cells=True)
    hip_engine.sync()
    assert_same(dev, host, 0, cells=True)
    sample = [0, 22_763, 22_764, 29_999]
    want = adaptive.adaptive_prefix(pool[sample], tr[sample], cap, need, flags, tokens=tok[sample], want_cells=True)
    assert np.array_equal(host.cells[sample], want.cells) and np.array_equal(host.cell_tokens[sample], want.cell_tokens)
    assert np.array_equal(host.cell_votes[sample], want.cell_votes)
    assert (host.stop_hist.sum(axis=1) == P).all()
    bad = pool.copy()
    bad[29_000, 3] = -4                                                 # only the second chunk holds it
    with pytest.raises(_lib.DomainError):
        hip_engine.adaptive_prefix(bad, tr, cap, need, flags, tokens=tok)


def test_tie_and_stop_counters_do_not_wrap(hip_engine, grid_option):
    """One workgroup, 3 (2^31 - 1) lanes; each stops rule 1 (cap 0) at n = 0 and rule 0 (cap 1, `never`) at n = 1 with a hit of one mode:
    one tie counter and two stop counters take 3 R > 2^32 increments, and a 32-bit LDS counter would wrap to 2^31 - 3.  The expected values
    are worked out by hand: the mirror cannot run 6.4e9 orderings."""
    R = 2 ** 31 - 1
    pool = np.full((3, 1), 4, dtype=np.int32)
    tok = np.ones((3, 1), dtype=np.int32)
    tr = np.full(3, 4, dtype=np.int32)
    cap = np.array([1, 0], dtype=np.int32)
    need = np.tile(never(1), (2, 1))
    grid_option(1)
    t0 = time.perf_counter()
    dp, dt, dtr, dc, dn = to_dev(pool, tok, tr, cap, need)
    tie, ts, vs, tcs, hist, per, _, _, _ = hip_engine.adaptive_prefix_device(dp, dtr, dc, dn, None, tokens=dt, r_begin=0, r_end=R, seed=5)
    hip_engine.sync()
    print(f"\nadaptive overflow test: {time.perf_counter() - t0:.1f} s")
    tie, hist = tie.cpu().numpy(), hist.cpu().numpy()
    assert per is None
    assert int(tie[0, 1]) == 3 * R and int(tie[0].sum()) == 3 * R and int(tie[1].sum()) == 0
    want_hist = np.zeros((2, 2), dtype=np.int64)
    want_hist[0, 1] = want_hist[1, 0] = 3 * R
    assert np.array_equal(hist, want_hist)
    for s in (vs, tcs, ts):
        assert s.cpu().numpy().tolist() == [3 * R, 0]


def test_slices_and_shards_add_up_on_the_device(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 100, 9, 4)
    cap, need, flags = rules_for(100, 6, 9)
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_begin=3, r_end=203, seed=11, M=101)
    dp, dt, dtr, dc, dn, df = to_dev(pool, tok, tr, cap, need, flags)
    out = eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=3, r_end=80, seed=11)
    eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=80, r_end=203, seed=11, tie_class_hits=out[0], token_sum=out[1],
                               vote_count_sum=out[2], truth_count_sum=out[3], stop_hist=out[4])
    per = torch.zeros((200, 6, 101), dtype=torch.int64, device=dp.device)
    shard = None
    for lo, hi in ((0, 4), (4, 11)):                                    # problem shards, each with its global offset
        s = eng.adaptive_prefix_device(dp[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dc, dn, df, tokens=dt[lo:hi].contiguous(), r_begin=3,
                                       r_end=203, seed=11, p_offset=lo, per_resample=per,
                                       **({} if shard is None else dict(tie_class_hits=shard[0], token_sum=shard[1], vote_count_sum=shard[2],
                                                                        truth_count_sum=shard[3], stop_hist=shard[4])))
        shard = s
    eng.sync()
    assert_same(out[:5] + (per, None, None, None), want, 101)
    assert_same(shard[:5] + (per, None, None, None), want, 101)
    whole = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True)
    assert_host_same(eng.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True), whole, 0, cells=True)
    a = eng.adaptive_prefix(pool[:4], tr[:4], cap, need, flags, tokens=tok[:4], want_cells=True)
    b = eng.adaptive_prefix(pool[4:], tr[4:], cap, need, flags, tokens=tok[4:], want_cells=True)
    assert np.array_equal(a.tie_class_hits + b.tie_class_hits, whole.tie_class_hits)
    assert np.array_equal(a.stop_hist + b.stop_hist, whole.stop_hist)
    assert np.array_equal(np.concatenate([a.cells, b.cells]), whole.cells)


def test_host_overwrites_device_accumulates_and_graph_replay():
    import torch
    pool, tok, tr = pool_of(20, 128, 33, 1)
    cap, need, flags = rules_for(128, 8, 33)
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=100, seed=4, M=129)
    dp, dt, dtr, dc, dn, df = to_dev(pool, tok, tr, cap, need, flags)
    twice = type(want)(want.P, want.R, 2 * want.tie_class_hits, 2 * want.token_sum, 2 * want.vote_count_sum, 2 * want.truth_count_sum,
                       2 * want.stop_hist, 2 * want.per_resample)
    with Engine(device=0) as eng:                                       # no SCV_FLAG_TIMING: no event records in the graph
        for _ in range(2):                                              # HOST: the same answer twice, not twice the answer
            assert_host_same(eng.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=100, seed=4, M=129), want, 129)
        got = eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=0, r_end=100, seed=4, M=129)
        keys = ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "stop_hist", "per_resample")
        eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=0, r_end=100, seed=4, **dict(zip(keys, got[:6])))
        eng.sync()
        assert_same(got, twice, 129)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got[:6]]
        kw = dict(zip(keys, bufs))
        with torch.cuda.stream(side):                                   # warm-up on the capture stream
            eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=0, r_end=100, seed=4, **kw)
        torch.cuda.synchronize()
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.adaptive_prefix_device(dp, dtr, dc, dn, df, tokens=dt, r_begin=0, r_end=100, seed=4, **kw)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        eng.sync()
        assert_same(bufs + [None, None, None], twice, 129)


def test_out_of_domain_votes_and_the_clamp_flag(hip_engine):
    pool, tok, tr = pool_of(4, 20, 21, 3)
    pool[1, 3], pool[2, 0] = -1, 4096
    tr[2] = 1023
    cap, need, flags = rules_for(20, 5, 21)
    with pytest.raises(_lib.DomainError):
        hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok)
    hip_engine.adaptive_prefix_device(*to_dev(pool, tr, cap, need, flags), r_begin=0, r_end=30, seed=1)
    with pytest.raises(_lib.DomainError):
        hip_engine.sync()
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=30, seed=1, M=21)
    assert want.error_bits & 1
    with Engine(device=0, clamp_to_invalid_bin=True) as ce:
        assert_host_same(ce.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=30, seed=1, M=21), want, 21)
        cells = ce.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True)
        assert_host_same(cells, adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, want_cells=True), 0, cells=True)


def test_negative_tokens_are_not_an_error(hip_engine):
    pool, tok, tr = pool_of(4, 20, 22, 1)
    tok[3, 19], tok[0, 0] = -1, -7
    cap, need, flags = rules_for(20, 4, 22)
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=7, seed=2, M=21)
    assert_host_same(hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=7, seed=2), want, 21)


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(8, dtype=np.int32), (3, 1))               # the whole pool is an 8-way tie
    tr = np.array([0, 1, 2], dtype=np.int32)
    cap, need = np.array([8], dtype=np.int32), never(8)[None, :]
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.adaptive_prefix(pool, tr, cap, need, resamples=5, M=8)
    assert ei.value.code == _lib.ERR_ARG
    out = hip_engine.adaptive_prefix_device(*to_dev(pool, tr, cap, need), r_begin=0, r_end=5, seed=1, M=4)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    assert int(out[0].cpu().numpy()[0, 8]) == 15                        # the tie-class table itself is complete
    hip_engine.sync()


def test_unknown_rule_flags(hip_engine):
    pool, tok, tr = pool_of(4, 20, 23, 1)
    cap, need = np.array([20, 20], dtype=np.int32), np.tile(never(20), (2, 1))
    for flags in ([0, 2], [3, 0], [0, -2 ** 31]):
        fl = np.array(flags, dtype=np.int32)
        with pytest.raises(_lib.ScvError) as ei:                        # HOST mode: at the call
            hip_engine.adaptive_prefix(pool, tr, cap, need, fl, resamples=3)
        assert ei.value.code == _lib.ERR_ARG and "rule_flags" in str(ei.value)
        hip_engine.adaptive_prefix_device(*to_dev(pool, tr, cap, need, fl), r_begin=0, r_end=3, seed=1)
        with pytest.raises(_lib.ScvError) as ei:                        # DEVICE mode: error bit 6 at sync
            hip_engine.sync()
        assert ei.value.code == _lib.ERR_ARG and "SCV_STOP_DECIDED" in str(ei.value)
        hip_engine.sync()                                               # the word was cleared


def test_bad_arguments_are_refused_at_the_call(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 300), dtype=np.int32)
    tok = np.zeros((2, 300), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    cap = np.ones(40, dtype=np.int32)
    need = np.ones((40, 301), dtype=np.int32)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    hist = np.zeros((40, 301), dtype=np.int64)
    cells = np.zeros(600 * 16, dtype=np.uint8)
    votes = np.zeros(600, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, order=1, r0=0, r1=4, p_off=0, M=1, per=None, capp=cap, needp=need, flagsp=None, tiep=tie, tokp=tok, ts=sums, c=None,
             ct=None, cv=None, mem=_lib.MEM_HOST, poolp=pool):
        return L.scv_adaptive_prefix_i32(ctx, ptr(poolp), ptr(tokp), ptr(capp), ptr(needp), ptr(flagsp), ptr(tr), 2, B, N, p_off, order, r0, r1,
                                         1, M, mem, ptr(tiep), ptr(ts), ptr(sums), ptr(sums), ptr(hist), ptr(per), ptr(c), ptr(ct), ptr(cv))
    assert call() == _lib.OK
    assert call(tokp=None, ts=None) == _lib.OK
    assert call(order=0, r0=0, r1=1, c=cells, ct=sums, cv=votes) == _lib.OK
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=33), dict(order=2), dict(order=-1), dict(order=0), dict(order=0, r0=1, r1=2),
               dict(order=0, r0=0, r1=0), dict(c=cells), dict(ct=sums), dict(cv=votes), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1),
               dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(capp=None), dict(needp=None), dict(tiep=None), dict(poolp=None),
               dict(tokp=None), dict(order=0, r0=0, r1=1, tokp=None, ts=None, ct=sums), dict(mem=7),
               dict(flagsp=np.array([0, 4], dtype=np.int32))):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"adaptive" in L.scv_last_error() or kw == dict(mem=7), kw


def test_empty_host_calls_overwrite_every_output(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    cap = np.ones(2, dtype=np.int32)
    need = np.ones((2, 9), dtype=np.int32)
    tie = np.full((2, 1025), -1, dtype=np.int64)
    sums = np.full(2, -1, dtype=np.int64)
    hist = np.full((2, 9), -1, dtype=np.int64)
    per = np.full((3, 2, 4), -1, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    assert L.scv_adaptive_prefix_i32(ctx, None, None, ptr(cap), ptr(need), None, None, 0, 2, 8, 0, _lib.ORDER_SHUFFLED, 0, 3, 1, 4,
                                     _lib.MEM_HOST, ptr(tie), None, ptr(sums), ptr(sums), ptr(hist), ptr(per), None, None, None) == _lib.OK
    assert not tie.any() and not sums.any() and not hist.any() and not per.any()


def test_the_reference_shape_and_the_curve(hip_engine):
    P, N, R = 30, 128, 200
    pool, tok, tr = pool_of(P, N, 2025, 1)
    rules = [(N, never(N), 0), (N, margin_rule(N, 2), 0), (N, margin_rule(N, 4), 0), (N, margin_rule(N, 8), 0), (N, beta_rule(N, 0.9), 0),
             (N, beta_rule(N, 0.95), 0), (N, beta_rule(N, 0.99), 0), (N, never(N), STOP_DECIDED)]
    cap = np.array([c for c, _n, _f in rules], dtype=np.int32)
    need = np.stack([n for _c, n, _f in rules])
    flags = np.array([f for _c, _n, f in rules], dtype=np.int32)
    got = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=R, seed=17, M=0)
    want = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=R, seed=17)
    assert_host_same(got, want, 0)
    recs = curves.adaptive_vote_records(hip_engine, pool, tr, tok, rules, resamples=R, seed=17)
    assert [r["accuracy"] for r in recs] == [got.accuracy(b) for b in range(8)]
    assert [r["avg_votes"] for r in recs] == [float(got.avg_votes(b)) for b in range(8)]
    assert [r["avg_tokens_used"] for r in recs] == [float(got.avg_tokens_used(b)) for b in range(8)]
    assert recs[0]["avg_votes"] == N and all(r["avg_votes"] <= N for r in recs)
    assert recs[7]["accuracy"] == recs[0]["accuracy"] and recs[7]["avg_votes"] < N
    assert recs[1]["avg_votes"] <= recs[2]["avg_votes"] <= recs[3]["avg_votes"]
    one = curves.adaptive_vote_records(hip_engine, pool, tr, tok, rules)
    pool_order = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok)
    assert [r["accuracy"] for r in one] == [pool_order.accuracy(b) for b in range(8)]
