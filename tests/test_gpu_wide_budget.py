"""GPU tests of scv_token_budget_wide_i32 (the vote over the longest prefix of an ordering of a pool of up to 4096 samples that fits a token
budget): every output bit-exact against the CPU mirror (o1_inference_scaling_laws_amd/wide_budget.py) in HOST and DEVICE mode, shuffled and
pool order, flag off and SCV_FLAG_OPEN_DOMAIN, across the pad boundaries of the sort, the chunk and wave edges of the scan and the workgroup
sizes; the identities with scv_token_budget_prefix_i32 (pool order) and scv_resample_wide_i32 (equal tokens); slices, shards, accumulation, a
captured graph, guard words, refusals, and a seeded sweep of 60 draws.  All comparisons are on integers."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, synth, wide, wide_budget
from o1_inference_scaling_laws_amd.engine import CELL_DTYPE, Engine, cells_from_torch, decode_min_mode

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024, 1025, 4095, 4096]
FIELDS = ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum")


@pytest.fixture(scope="module")
def open_engine():
    with Engine(device=0, open_domain=True) as eng:
        yield eng


def pool_of(P, N, seed, dist):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    return a[:, 0, :].copy(), t[:, 0, :].copy(), tr


def spread(x):
    """A relabelling of small integers over the whole int32 range that keeps equality (odd multiplier mod 2^32)."""
    return ((np.asarray(x).astype(np.int64) * 2654435761 + 12345) % (1 << 32) - (1 << 31)).astype(np.int32)


def budgets_of(tok, k=0):
    """Unsorted; always a duplicate pair, a negative budget, 0, one beyond the row's total and one inside the first samples in front; ``k``
    varies B by trimming the tail."""
    total = int(tok.astype(np.int64).sum(axis=1).max())
    few = int(tok[0, :3].astype(np.int64).sum())
    out = [total // 2, -3 - k, total + 1, 0, total // 2, few, total // 7, total // 50, 1 << 62, total - 1]
    return np.array(out[:len(out) - k % 3], dtype=np.int64)


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def same_result(got, want, cells=False):
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    if want.per_resample is not None:
        assert np.array_equal(got.per_resample, want.per_resample)
    if cells:
        assert got.cells.tobytes() == want.cells.tobytes()
        assert np.array_equal(got.cell_tokens, want.cell_tokens)


def same_device(bufs, want, cells=False, times=1):
    tie, ts, vs, tcs, per, dc, dct = bufs
    assert np.array_equal(tie.cpu().numpy(), times * want.tie_class_hits)
    assert np.array_equal(ts.cpu().numpy(), times * want.token_sum)
    assert np.array_equal(vs.cpu().numpy(), times * want.vote_count_sum)
    assert np.array_equal(tcs.cpu().numpy(), times * want.truth_count_sum)
    if want.per_resample is not None:
        assert np.array_equal(per.cpu().numpy(), times * want.per_resample)
    if cells:                                                             # overwritten, never accumulated
        assert cells_from_torch(dc).tobytes() == want.cells.tobytes()
        assert np.array_equal(dct.cpu().numpy(), want.cell_tokens)


def check_all_four(eng, pool, tok, tr, budgets, R, r0, seed, p_off, M, open_domain):
    """HOST and DEVICE, shuffled and pool order, every output requested."""
    for shuffled in (True, False):
        r1 = r0 + R if shuffled else None
        rb = r0 if shuffled else 0
        want = wide_budget.token_budget_wide(pool, tok, tr, budgets, rb, r1, seed=seed, p_offset=p_off, M=M, want_cells=not shuffled,
                                             open_domain=open_domain)
        assert want.error_bits == 0
        got = eng.token_budget_wide(pool, tok, tr, budgets, resamples=R if shuffled else None, seed=seed, r_begin=rb, p_offset=p_off, M=M,
                                    want_cells=not shuffled)
        same_result(got, want, cells=not shuffled)
        dp, dt, dtr, db = to_dev(pool, tok, tr, budgets)
        bufs = eng.token_budget_wide_device(dp, dt, dtr, db, rb, r1, seed, p_offset=p_off, M=M, want_cells=not shuffled)
        eng.sync()
        same_device(bufs, want, cells=not shuffled)


@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(hip_engine, N):
    k = NS.index(N)
    P, R = (2, 3) if N >= 4095 else (2 + k % 5, 1 + k % 5)
    pool, tok, tr = pool_of(P, N, 300 + k, k % 6)
    if k % 4 == 1:
        tr[0] = -7                                                        # a truth outside the bins never hits
    check_all_four(hip_engine, pool, tok, tr, budgets_of(tok, k), R, (0, 7, 2 ** 31 - 1 - R)[k % 3], 4000 + k, (0, 5, 1 << 33)[(k + 1) % 3],
                   min(N, 1024) + 1, False)


@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror_open_domain(open_engine, N):
    k = NS.index(N)
    P, R = (2, 3) if N >= 4095 else (2 + (k + 2) % 5, 1 + (k + 3) % 5)
    pool, tok, tr = pool_of(P, N, 500 + k, (k + 1) % 6)
    pool, tr = spread(pool), spread(tr)
    if N == 4096:
        # a row of more than 1024 distinct values (1 + 1400), none of them twice in a row of the cache: every third sample is one dominant
        # value, the truth, so no prefix reaches a 1025-way tie (an error, tested below) and no budget has to be capped
        i = np.arange(N)
        pool[1] = spread(np.where(i % 3 == 0, 7, 3000 + i % 1400))
        tr[1] = pool[1, 0]
        assert len(np.unique(pool[1])) > 1024
    budgets = budgets_of(tok, k)
    check_all_four(open_engine, pool, tok, tr, budgets, R, (0, 7, 2 ** 31 - 1 - R)[k % 3], 4100 + k, (0, 5, 1 << 33)[(k + 1) % 3],
                   min(N, 1024) + 1, True)


def test_decode_min_mode_round_trips_in_pool_order(open_engine):
    import statistics
    pool, tok, tr = pool_of(5, 700, 61, 3)
    pool, tr = spread(pool), spread(tr)
    budgets = budgets_of(tok)
    got = open_engine.token_budget_wide(pool, tok, tr, budgets, want_cells=True)
    vals = decode_min_mode(pool, got.cells)
    run = np.cumsum(tok.astype(np.int64), axis=1)
    for p in range(5):
        for b, T in enumerate(budgets.tolist()):
            n = int(np.searchsorted(run[p], T, side="right"))
            assert vals[p, b] == (min(statistics.multimode(pool[p, :n].tolist())) if n else -1), (p, b)


def test_flag_on_equals_flag_off_inside_the_bins(hip_engine, open_engine):
    pool, tok, tr = pool_of(4, 900, 71, 1)
    assert pool.min() >= 0 and pool.max() <= 1023
    budgets = budgets_of(tok)
    for resamples in (None, 4):
        a = hip_engine.token_budget_wide(pool, tok, tr, budgets, resamples=resamples, seed=3, want_cells=resamples is None)
        b = open_engine.token_budget_wide(pool, tok, tr, budgets, resamples=resamples, seed=3, want_cells=resamples is None)
        for f in FIELDS + ("per_resample",):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        if resamples is None:
            assert np.array_equal(a.cell_tokens, b.cell_tokens)
            for f in ("max_count", "truth_count", "n_modes", "hit"):
                assert np.array_equal(a.cells[f], b.cells[f]), f
            assert np.array_equal(decode_min_mode(pool, b.cells), a.cells["min_mode"].astype(np.int64))


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("N", [1, 5, 64, 200, 256])
def test_pool_order_equals_the_prefix_entry_in_every_output(hip_engine, open_engine, N, flag):
    eng = open_engine if flag else hip_engine
    pool, tok, tr = pool_of(6, N, 80 + N, 1 if N % 2 else 3)
    if flag:
        pool, tr = spread(pool), spread(tr)
    budgets = budgets_of(tok, N)
    a = eng.token_budget_wide(pool, tok, tr, budgets, want_cells=True)
    b = eng.token_budget_prefix(pool, tok, tr, budgets, want_cells=True)
    same_result(a, b, cells=True)


@pytest.mark.parametrize("N", [300, 1024])
def test_equal_tokens_reduce_to_resample_wide(hip_engine, N):
    P, R, c = 4, 5, 37
    pool, _, tr = pool_of(P, N, 90 + N, 1)
    tok = np.full((P, N), c, dtype=np.int32)
    ks = np.array([1, 2, N // 3, N - 1, N, 17, 17, 0], dtype=np.int64)
    a = hip_engine.token_budget_wide(pool, tok, tr, c * ks + (c - 1), resamples=R, seed=9, r_begin=2, p_offset=1, M=0)
    w = hip_engine.resample_wide(pool, tr, ks.astype(np.int32), R, 9, tokens=tok, r_begin=2, p_offset=1, M=0)
    assert np.array_equal(a.tie_class_hits, w.tie_class_hits) and np.array_equal(a.truth_count_sum, w.truth_count_sum)
    assert np.array_equal(a.token_sum, w.token_sum) and np.array_equal(a.vote_count_sum, P * R * ks)


@pytest.mark.parametrize("grid,P,R", [(0, 1, 1), (7, 3, 5)])
def test_fewer_and_more_items_than_workgroups(grid, P, R):
    """One item on a full grid; 15 items on 7 workgroups: a run of three items crosses the end of a problem (5 items each)."""
    N = 333
    pool, tok, tr = pool_of(P, N, 44, 3)
    budgets = budgets_of(tok)
    want = wide_budget.token_budget_wide(pool, tok, tr, budgets, 1, 1 + R, seed=6, M=N + 1)
    with Engine(device=0) as eng:
        if grid:
            eng.set_option("grid", grid)
        same_result(eng.token_budget_wide(pool, tok, tr, budgets, resamples=R, seed=6, r_begin=1, M=N + 1), want)
        if P > 1:                                                         # pool order too: three problems on seven workgroups, and on one
            wp = wide_budget.token_budget_wide(pool, tok, tr, budgets, want_cells=True, M=N + 1)
            same_result(eng.token_budget_wide(pool, tok, tr, budgets, want_cells=True, M=N + 1), wp, cells=True)
            eng.set_option("grid", 1)
            same_result(eng.token_budget_wide(pool, tok, tr, budgets, want_cells=True, M=N + 1), wp, cells=True)
            same_result(eng.token_budget_wide(pool, tok, tr, budgets, resamples=R, seed=6, r_begin=1, M=N + 1), want)


def test_slices_shards_accumulation_and_overwritten_cells(hip_engine):
    import torch
    eng = hip_engine
    P, N, B = 6, 530, 7
    pool, tok, tr = pool_of(P, N, 9, 4)
    budgets = budgets_of(tok)[:B]
    want = wide_budget.token_budget_wide(pool, tok, tr, budgets, 3, 8, seed=11, M=N + 1)
    dp, dt, dtr, db = to_dev(pool, tok, tr, budgets)
    bufs = eng.token_budget_wide_device(dp, dt, dtr, db, 3, 5, 11)                           # slices of r into one set of buffers
    eng.token_budget_wide_device(dp, dt, dtr, db, 5, 8, 11, tie_class_hits=bufs[0], token_sum=bufs[1], vote_count_sum=bufs[2], truth_count_sum=bufs[3])
    per = torch.zeros((5, B, N + 1), dtype=torch.int64, device=dp.device)
    sh = None
    for lo, hi in ((0, 2), (2, 6)):                                                          # shards of p, each with its global offset
        sh = eng.token_budget_wide_device(dp[lo:hi].contiguous(), dt[lo:hi].contiguous(), dtr[lo:hi].contiguous(), db, 3, 8, 11, p_offset=lo,
                                          per_resample=per, **({} if sh is None else dict(tie_class_hits=sh[0], token_sum=sh[1],
                                                                                          vote_count_sum=sh[2], truth_count_sum=sh[3])))
    eng.sync()
    same_device(bufs[:4] + (None, None, None), _without_per(want))
    same_device(sh[:4] + (per, None, None), want)
    # DEVICE mode accumulates: two calls give twice the counters; the cells are overwritten
    wp = wide_budget.token_budget_wide(pool, tok, tr, budgets, M=N + 1, want_cells=True)
    two = eng.token_budget_wide_device(dp, dt, dtr, db, M=N + 1, want_cells=True)
    two[5].fill_(0xAB)
    two[6].fill_(-1)
    eng.token_budget_wide_device(dp, dt, dtr, db, tie_class_hits=two[0], token_sum=two[1], vote_count_sum=two[2], truth_count_sum=two[3],
                                 per_resample=two[4], cells=two[5], cell_tokens=two[6])
    eng.sync()
    same_device(two, wp, cells=True, times=2)


def _without_per(res):
    import copy
    out = copy.copy(res)
    out.per_resample = None
    return out


def test_a_captured_graph_replayed_twice():
    import torch
    pool, tok, tr = pool_of(4, 1500, 33, 1)
    budgets = budgets_of(tok)
    want = wide_budget.token_budget_wide(pool, tok, tr, budgets, 0, 5, seed=4, M=1025)
    dp, dt, dtr, db = to_dev(pool, tok, tr, budgets)
    with Engine(device=0) as eng:                                          # no SCV_FLAG_TIMING: no event records in the graph
        got = eng.token_budget_wide_device(dp, dt, dtr, db, 0, 5, 4, M=1025)
        eng.sync()
        same_device(got, want)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got[:5]]
        kw = dict(tie_class_hits=bufs[0], token_sum=bufs[1], vote_count_sum=bufs[2], truth_count_sum=bufs[3], per_resample=bufs[4])
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
            eng.token_budget_wide_device(dp, dt, dtr, db, 0, 5, 4, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.token_budget_wide_device(dp, dt, dtr, db, 0, 5, 4, **kw)
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g.replay()
        g.replay()                                                         # replayed twice: DEVICE mode accumulates
        torch.cuda.synchronize()
        eng.sync()
        same_device(tuple(bufs) + (None, None), want, times=2)


def test_guard_words_around_the_device_outputs(hip_engine):
    import torch
    eng = hip_engine
    P, N, B, G = 3, 1025, 5, 16
    pool, tok, tr = pool_of(P, N, 17, 1)
    budgets = budgets_of(tok)[:B]
    want = wide_budget.token_budget_wide(pool, tok, tr, budgets, want_cells=True, M=8)
    dp, dt, dtr, db = to_dev(pool, tok, tr, budgets)
    SENT = 0x5A5A5A5A5A5A5A5A
    sizes = {"tie": B * 1025, "ts": B, "vs": B, "tcs": B, "per": B * 8, "ctok": P * B, "cells": P * B * 2}
    big = torch.full((sum(sizes.values()) + G * (len(sizes) + 1),), SENT, dtype=torch.int64, device=dp.device)
    views, at = {}, G
    for name, n in sizes.items():
        views[name] = big[at:at + n]
        views[name].zero_()
        at += n + G
    keep = big.clone()
    cells = views["cells"].view(torch.uint8).view(P, B, 16)
    out = eng.token_budget_wide_device(dp, dt, dtr, db, tie_class_hits=views["tie"].view(B, 1025), token_sum=views["ts"], vote_count_sum=views["vs"],
                                       truth_count_sum=views["tcs"], per_resample=views["per"].view(1, B, 8), cells=cells,
                                       cell_tokens=views["ctok"].view(P, B))
    eng.sync()
    same_device(out, want, cells=True)
    mask = torch.ones_like(big, dtype=torch.bool)
    at = G
    for n in sizes.values():
        mask[at:at + n] = False
        at += n + G
    assert int(mask.sum()) == G * (len(sizes) + 1) and torch.equal(big[mask], keep[mask])
    assert bool((big[mask] == SENT).all())


def test_refusals(hip_engine):
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 4100), dtype=np.int32)
    tok = np.ones((2, 4100), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    bud = np.ones(40, dtype=np.int64)
    tie = np.zeros((40, 1025), dtype=np.int64)
    sums = np.zeros(40, dtype=np.int64)
    cells = np.zeros((2, 40), dtype=CELL_DTYPE)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, order=_lib.ORDER_SHUFFLED, r0=0, r1=4, p_off=0, M=1, tokp=tok, budp=bud, tiep=tie, per=None, cellp=None, ctokp=None):
        return L.scv_token_budget_wide_i32(ctx, ptr(pool), ptr(tokp), ptr(budp), ptr(tr), 2, B, N, p_off, order, r0, r1, 1, M, _lib.MEM_HOST,
                                           ptr(tiep), ptr(sums), ptr(sums), ptr(sums), ptr(per), ptr(cellp), ptr(ctokp))
    assert call() == _lib.OK
    assert call(N=4096) == _lib.OK
    assert call(order=_lib.ORDER_POOL, r0=0, r1=1, cellp=cells, ctokp=np.zeros((2, 40), dtype=np.int64)) == _lib.OK
    for kw in (dict(tokp=None), dict(budp=None), dict(tiep=None), dict(order=2), dict(order=-1), dict(order=_lib.ORDER_POOL), dict(order=_lib.ORDER_POOL, r0=1, r1=2),
               dict(order=_lib.ORDER_POOL, r0=0, r1=2), dict(cellp=cells), dict(ctokp=np.zeros((2, 40), dtype=np.int64)), dict(N=0), dict(N=4097), dict(B=0),
               dict(B=33), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1), dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"token_budget_wide" in L.scv_last_error(), kw
    assert call() == _lib.OK


def test_negative_tokens_and_too_few_classes(hip_engine):
    eng = hip_engine
    pool, tok, tr = pool_of(3, 400, 23, 1)
    budgets = budgets_of(tok)
    bad = tok.copy()
    bad[1, 399] = -1
    for resamples in (None, 3):
        with pytest.raises(_lib.ScvError) as ei:
            eng.token_budget_wide(pool, bad, tr, budgets, resamples=resamples)
        assert ei.value.code == _lib.ERR_ARG
    dp, dt, dtr, db = to_dev(pool, bad, tr, budgets)
    eng.token_budget_wide_device(dp, dt, dtr, db, 0, 3, 1)
    with pytest.raises(_lib.ScvError) as ei:
        eng.sync()
    assert ei.value.code == _lib.ERR_ARG
    eng.sync()                                                             # the word was cleared: the context works again
    same_result(eng.token_budget_wide(pool, tok, tr, budgets, resamples=2, seed=5, M=401),
                wide_budget.token_budget_wide(pool, tok, tr, budgets, 0, 2, seed=5, M=401))
    # per_resample with too few classes: bit 1
    flat = np.tile(np.arange(300, dtype=np.int32), (2, 1))                # every prefix is an all-way tie: n_modes == n
    one = np.ones((2, 300), dtype=np.int32)
    t0 = np.zeros(2, dtype=np.int32)
    with pytest.raises(_lib.ScvError) as ei:
        eng.token_budget_wide(flat, one, t0, [300], M=300)
    assert ei.value.code == _lib.ERR_ARG
    dp, dt, dtr, db = to_dev(flat, one, t0, np.array([300], dtype=np.int64))
    tie = eng.token_budget_wide_device(dp, dt, dtr, db, M=4)[0]
    with pytest.raises(_lib.ScvError):
        eng.sync()
    assert int(tie.cpu().numpy()[0, 300]) == 2                             # the tie-class table itself is complete: one 300-way tie per problem
    eng.sync()


def test_a_1025_way_tie_has_no_column_on_the_gpu(open_engine):
    """Open domain, all values distinct: a prefix of n samples ties n ways.  The hit of 1025 ways sets error bit 1 (SCV_ERR_ARG: at the call in
    HOST mode, at scv_sync in DEVICE mode) and is counted in neither table; its sums are still added, and every other budget is complete."""
    eng = open_engine
    P, N, R = 2, 2100, 2
    pool = spread(np.arange(P * N).reshape(P, N))
    tok = np.ones((P, N), dtype=np.int32)
    tr = pool[:, 0].copy()
    budgets = np.array([1024, 1025, 5, 2100], dtype=np.int64)
    dp, dt, dtr, db = to_dev(pool, tok, tr, budgets)
    for r_end in (None, R):                                               # pool order (the truth is sample 0: every prefix hits), then shuffled
        want = wide_budget.token_budget_wide(pool, tok, tr, budgets, 0, r_end, seed=3, M=1025, want_cells=r_end is None, open_domain=True)
        assert want.error_bits == 2 and want.vote_count_sum.tolist() == [x * P * (r_end or 1) for x in (1024, 1025, 5, 2100)]
        with pytest.raises(_lib.ScvError) as ei:
            eng.token_budget_wide(pool, tok, tr, budgets, resamples=r_end, seed=3, M=1025, want_cells=r_end is None)
        assert ei.value.code == _lib.ERR_ARG
        bufs = eng.token_budget_wide_device(dp, dt, dtr, db, 0, r_end, 3, M=1025, want_cells=r_end is None)
        with pytest.raises(_lib.ScvError) as ei:
            eng.sync()
        assert ei.value.code == _lib.ERR_ARG
        same_device(bufs, want, cells=r_end is None)
        assert int(bufs[0].cpu().numpy()[1].sum()) == 0 and int(bufs[4].cpu().numpy()[:, 1].sum()) == 0
    assert int(bufs[0].cpu().numpy()[3].sum()) == 0                       # (2100 ways: no column either)
    eng.sync()                                                            # the word was cleared


FUZZ_SEED = 20261020
FUZZ_NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 777, 1000, 1024, 1025, 2048, 2049, 4095, 4096)


def fuzz_draws():
    """60 draws of (N, P, R or None for pool order, B, flag, mode, token scale, seeds)."""
    rng = np.random.default_rng(FUZZ_SEED)
    draws = []
    for i in range(60):
        N = int(FUZZ_NS[int(rng.integers(len(FUZZ_NS)))])
        big = N > 1025
        draws.append(dict(N=N, P=int(rng.integers(1, 3 if big else 5)), R=None if rng.integers(3) == 0 else int(rng.integers(1, 3 if big else 6)),
                          B=int(rng.integers(1, 13)), flag=bool(rng.integers(2)), device=bool(rng.integers(2)),
                          scale=("zero", "one", "synth", "synth", "large", "max")[int(rng.integers(6))], dist=int(rng.integers(6)),
                          seed=int(rng.integers(1 << 40)), r0=int(rng.integers(0, 50)), p_off=int(rng.integers(0, 1 << 34)), i=i))
    return draws


def fuzz_inputs(d):
    rng = np.random.default_rng(d["seed"])
    pool, tok, tr = pool_of(d["P"], d["N"], d["seed"] % 10007, d["dist"])
    if d["flag"]:
        pool, tr = spread(pool), spread(tr)
    t64 = tok.astype(np.int64)
    tok = {"zero": 0 * t64, "one": 0 * t64 + 1, "synth": t64, "large": np.minimum(t64 * 100003, 2 ** 31 - 1), "max": 0 * t64 + 2 ** 31 - 1}[d["scale"]].astype(np.int32)
    total = int(tok.astype(np.int64).sum(axis=1).max())
    menu = [total, total + 1, 1 << 62, 0, -1, -(1 << 62), total // 2, total // 3, total // 9, int(tok[0, :5].astype(np.int64).sum()),
            int(tok[0, :40].astype(np.int64).sum()), total // 100, total - 1, int(rng.integers(0, total + 2))]
    budgets = np.array([menu[int(rng.integers(len(menu)))] for _ in range(d["B"])], dtype=np.int64)
    return pool, tok, tr, budgets


def fuzz_want(d, pool, tok, tr, budgets):
    r1 = None if d["R"] is None else d["r0"] + d["R"]
    return wide_budget.token_budget_wide(pool, tok, tr, budgets, 0 if d["R"] is None else d["r0"], r1, seed=d["seed"], p_offset=d["p_off"],
                                         M=min(d["N"], 1024) + 1, want_cells=d["R"] is None, open_domain=d["flag"])


def fuzz_prefix_lengths(d, tok, budgets):
    """n_b of every ordering of the draw, from the mirror's own pieces: int64 [P * R, B]."""
    N = d["N"]
    out = []
    for p in range(d["P"]):
        order = np.arange(N).reshape(1, N) if d["R"] is None else wide.orderings(d["seed"], d["p_off"] + p, np.arange(d["r0"], d["r0"] + d["R"]), N)
        out.append(wide_budget.prefix_lengths(tok[p].astype(np.int64)[order], budgets))
    return np.concatenate(out)


def test_seeded_fuzz_sweep(hip_engine, open_engine):
    cover = dict(wide=0, pool_cells=0, flag=0, short=0, whole=0, whole_wide_flag=0)
    for d in fuzz_draws():
        pool, tok, tr, budgets = fuzz_inputs(d)
        want = fuzz_want(d, pool, tok, tr, budgets)
        assert want.error_bits == 0, d                                     # every draw is compared: none is skipped
        cells = d["R"] is None
        den = want.P * want.R
        cover["wide"] += d["N"] > 256
        cover["pool_cells"] += cells
        cover["flag"] += d["flag"]
        n = fuzz_prefix_lengths(d, tok, budgets)                           # [P * R, B], one row per ordering
        cover["short"] += bool(d["N"] > 64 and ((n > 0) & (n < 64)).all(axis=0).any())      # a budget that ends inside the first 64 samples of every ordering
        whole = bool((n == d["N"]).all(axis=0).any())                      # a budget that takes the whole pool
        assert whole == bool((want.vote_count_sum == den * d["N"]).any())
        cover["whole"] += whole
        cover["whole_wide_flag"] += whole and d["flag"] and d["N"] > 256
        eng = open_engine if d["flag"] else hip_engine
        M = min(d["N"], 1024) + 1
        if d["device"]:
            dp, dt, dtr, db = to_dev(pool, tok, tr, budgets)
            bufs = eng.token_budget_wide_device(dp, dt, dtr, db, 0 if cells else d["r0"], None if cells else d["r0"] + d["R"], d["seed"],
                                                p_offset=d["p_off"], M=M, want_cells=cells)
            eng.sync()
            same_device(bufs, want, cells=cells)
        else:
            got = eng.token_budget_wide(pool, tok, tr, budgets, resamples=d["R"], seed=d["seed"], r_begin=0 if cells else d["r0"],
                                        p_offset=d["p_off"], M=M, want_cells=cells)
            same_result(got, want, cells=cells)
    assert cover["wide"] >= 15 and cover["pool_cells"] >= 10 and cover["flag"] >= 15 and cover["short"] >= 5 and cover["whole"] >= 5, cover
    assert cover["whole_wide_flag"] >= 3, cover                            # ... also with the flag on beyond 256 samples
