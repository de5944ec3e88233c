"""GPU tests of scv_shortest_prefix_i32 (short-m@k: the majority vote over the m shortest of the first k samples of a pool ordering): every
output bit-exact against the CPU mirror (o1_inference_scaling_laws_amd/shortest.py) in HOST and DEVICE mode and in both orders -- pool sizes
at the bitmap-word and register edges, partial chunks and rows shared by two waves, budget and token edges, the count byte at 256, slices,
shards, accumulation, a captured graph, the identities of the header, the open answer domain, the argument errors and a fuzz sweep."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, curves, shortest, synth
from o1_inference_scaling_laws_amd.engine import Engine, cells_from_torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 5, 31, 32, 33, 63, 64, 65, 128, 255, 256]
SUMS = ("tie_class_hits", "voted_token_sum", "spent_token_sum", "latency_sum", "truth_count_sum")


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def pool_of(P, N, seed, dist=1, tokens="synth"):
    """synth pools; tokens: the synthetic ones (100 .. 12 000), ``two`` distinct values, all ``equal``, or mostly ``zeros``."""
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    pool, tok = a[:, 0, :].copy(), t[:, 0, :].copy()
    rng = np.random.default_rng(seed)
    if tokens == "two":
        tok = rng.choice(np.array([40, 41], dtype=np.int32), size=pool.shape).astype(np.int32)
    elif tokens == "equal":
        tok = np.full_like(pool, 977)
    elif tokens == "zeros":
        tok = np.where(rng.random(pool.shape) < 0.8, 0, tok).astype(np.int32)
    return pool, tok, tr


def pairs_for(N, B, seed):
    """ragged, unsorted, duplicated: k = 0, k > N, m = 0, m < 0, m > k, (k, 1), (k, k / 4), (k, k)."""
    rng = np.random.default_rng(seed)
    base = [(0, 0), (0, 3), (N + 5, 1), (N, N), (N, 0), (N, -2), (1, 1), (max(N // 2, 1), N + 3), (N, max(N // 4, 1)), (N, N - 1)]
    base += [(int(k), int(rng.integers(-1, k + 2))) for k in rng.integers(0, N + 1, size=8)]
    pick = rng.integers(0, len(base), size=B)
    return np.array([base[i][0] for i in pick], dtype=np.int32), np.array([base[i][1] for i in pick], dtype=np.int32)


def assert_host_same(got, want, per=True, cells=False):
    for name in SUMS:
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    if per:
        assert np.array_equal(got.per_resample, want.per_resample)
    if cells:
        assert np.array_equal(got.cells, want.cells) and np.array_equal(got.cell_tokens, want.cell_tokens)


def assert_dev_same(got, want, per=True, cells=False, times=1):
    out = [None if x is None else x.cpu().numpy() for x in got]
    for x, name in zip(out[:5], SUMS):
        assert np.array_equal(x, times * getattr(want, name)), name
    if per:
        assert np.array_equal(out[5], times * want.per_resample)
    if cells:
        assert np.array_equal(cells_from_torch(got[6]), want.cells) and np.array_equal(out[7], want.cell_tokens)


def both_modes(eng, pool, tok, tr, nv, mk, r0, R, seed, p_off=0, open_domain=False):
    """mirror, DEVICE and HOST over one input, bit for bit; R None: pool order with cells."""
    N = pool.shape[1]
    M = N + 1
    shuffled = R is not None
    want = shortest.shortest_prefix(pool, tok, tr, nv, mk, r0, r0 + R if shuffled else None, seed, p_off, M=M, want_cells=not shuffled,
                                    open_domain=open_domain)
    assert want.error_bits == 0
    got = eng.shortest_prefix_device(*to_dev(pool, tok, tr, nv, mk), r0, r0 + R if shuffled else None, seed, p_offset=p_off, M=M,
                                     want_cells=not shuffled)
    eng.sync()
    assert_dev_same(got, want, cells=not shuffled)
    host = eng.shortest_prefix(pool, tok, tr, nv, mk, resamples=R, seed=seed, r_begin=r0, p_offset=p_off, M=M, want_cells=not shuffled)
    assert_host_same(host, want, cells=not shuffled)
    return want


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("N", NS)
def test_pool_sizes_bit_exact_against_the_mirror(hip_engine, N, shuffled):
    """bitmap words end at 32, 64, ...; the counting loop's registers at 64, 128, 192; rows of 1, 2, 5, 31, 33, 63, 65, 255 are no multiple of 4."""
    for draw, kind in enumerate(("synth", "two", "equal", "zeros")):
        k = NS.index(N) + draw
        B = (1, 8, 32)[k % 3]
        P, R = (3 + k % 3, (7, 65)[k % 2]) if shuffled else (5 + 30 * (k % 3), None)
        pool, tok, tr = pool_of(P, N, 40 + k, dist=k % 6, tokens=kind)
        nv, mk = pairs_for(N, B, k)
        both_modes(hip_engine, pool, tok, tr, nv, mk, (0, 7, 2 ** 31 - 1 - 65)[k % 3] if shuffled else 0, R, 2024 + k,
                   (0, 5, 1 << 33)[(k + 1) % 3])


@pytest.mark.parametrize("R", [1, 7, 65, 130])
@pytest.mark.parametrize("P", [1, 3, 30])
def test_shape_sweep(hip_engine, P, R):
    """partial chunks (P * R below and off the workgroup sizes) and rows shared by two waves (R = 65, 130); B = 1, and B = 32 with duplicates."""
    N = 65
    pool, tok, tr = pool_of(P, N, P * 1000 + R, dist=(P + R) % 6)
    nv, mk = pairs_for(N, 32, P + R)
    nv[5:9], mk[5:9] = nv[4], mk[4]                                       # duplicates for certain
    both_modes(hip_engine, pool, tok, tr, nv, mk, 3, R, 11)
    both_modes(hip_engine, pool, tok, tr, nv[:1] * 0 + 40, mk[:1] * 0 + 9, 0, R, 12)
    if R == 1:
        both_modes(hip_engine, pool, tok, tr, nv, mk, 0, None, 0)


def test_budget_edges(hip_engine):
    """k = 0, k > N, m = 0, m < 0, m > k, each where the mirror's clamps put it."""
    N = 33
    pool, tok, tr = pool_of(9, N, 5, dist=2)                             # every vote the truth: any non-empty V hits
    nv = np.array([0, 0, N + 9, 2 ** 31 - 1, 7, 7, 7, -4, 1], dtype=np.int32)
    mk = np.array([0, 5, 3, 2 ** 31 - 1, 0, -1, 99, 2, 1], dtype=np.int32)
    for R in (None, 70):
        want = both_modes(hip_engine, pool, tok, tr, nv, mk, 0, R, 3)
        cells = 9 * (R or 1)
        for b, (k, m) in enumerate([(0, 0), (0, 0), (N, 3), (N, N), (7, 0), (7, 0), (7, 7), (0, 0), (1, 1)]):
            assert int(want.tie_class_hits[b, 1]) == (cells if m else 0) and int(want.truth_count_sum[b]) == cells * m
            if not m:
                assert not want.spent_token_sum[b] and not want.latency_sum[b] and not want.voted_token_sum[b]
        if R is None:
            assert (want.cells["max_count"][:, [0, 1, 4, 5, 7]] == 0).all() and (want.cells["min_mode"][:, [0, 1, 4, 5, 7]] == -1).all()


def test_largest_tokens_keep_the_int64_product(hip_engine):
    """N = 256, every token 2^31 - 1, k = 256, m = 1: spent = (2^31 - 1) * 256 per cell, k - m = 255 of it the cut-off chains."""
    big = 2 ** 31 - 1
    pool, _, tr = pool_of(3, 256, 6)
    tok = np.full_like(pool, big)
    nv, mk = np.array([256, 256], dtype=np.int32), np.array([1, 256], dtype=np.int32)
    for R in (None, 5):
        want = both_modes(hip_engine, pool, tok, tr, nv, mk, 0, R, 8)
        cells = 3 * (R or 1)
        assert want.spent_token_sum.tolist() == [cells * big * 256] * 2 and want.voted_token_sum.tolist() == [cells * big, cells * big * 256]
        assert want.latency_sum.tolist() == [cells * big] * 2


def test_negative_tokens_are_an_argument_error(hip_engine):
    pool, tok, tr = pool_of(4, 20, 22)
    tok[3, 19] = -1
    nv, mk = np.array([20, 5], dtype=np.int32), np.array([3, 5], dtype=np.int32)
    assert shortest.shortest_prefix(pool, tok, tr, nv, mk).error_bits == 16
    for R in (None, 7):
        with pytest.raises(_lib.ScvError) as ei:
            hip_engine.shortest_prefix(pool, tok, tr, nv, mk, resamples=R)
        assert ei.value.code == _lib.ERR_ARG and "negative" in str(ei.value)
    hip_engine.shortest_prefix_device(*to_dev(pool, tok, tr, nv, mk), 0, 7, 1)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    hip_engine.sync()                                                   # the word was cleared


@pytest.mark.parametrize("shuffled", [False, True])
def test_256_equal_votes_reach_a_count_of_256(hip_engine, shuffled):
    """The byte edge: N = 256, one value everywhere, m = k = 256.  The count byte wraps to 0 at the last step; max_count is 256."""
    pool = np.full((2, 256), 17, dtype=np.int32)
    tr = np.array([17, 18], dtype=np.int32)
    tok = np.random.default_rng(1).integers(0, 5000, size=pool.shape).astype(np.int32)
    nv, mk = np.array([256, 256, 255], dtype=np.int32), np.array([256, 255, 255], dtype=np.int32)
    R = 6 if shuffled else None
    want = both_modes(hip_engine, pool, tok, tr, nv, mk, 0, R, 4)
    assert want.tie_class_hits[:, 1].tolist() == [R or 1] * 3 and want.truth_count_sum.tolist() == [256 * (R or 1), 255 * (R or 1), 255 * (R or 1)]
    if not shuffled:
        got = hip_engine.shortest_prefix(pool, tok, tr, nv, mk, want_cells=True)
        assert got.cells["max_count"][:, 0].tolist() == [256, 256] and got.cells["max_count"][:, 1].tolist() == [255, 255]
        assert got.cells["truth_count"][:, 0].tolist() == [256, 0] and got.cells["min_mode"][:, 0].tolist() == [17, 17]


def test_truth_absent_from_the_row(hip_engine):
    pool, tok, tr = pool_of(6, 64, 9, dist=1)
    tr[:] = [1022, 1023, 5000, -1, int(pool[4, 0]), 1021]                # in the bins but absent, outside the bins, present
    pool[pool >= 1021] = 0
    nv, mk = pairs_for(64, 8, 9)
    for R in (None, 66):
        want = both_modes(hip_engine, pool, tok, tr, nv, mk, 0, R, 2)
        alone = shortest.shortest_prefix(pool[4:5], tok[4:5], tr[4:5], nv, mk, 0, R, 2, p_offset=4)
        assert np.array_equal(want.tie_class_hits, alone.tie_class_hits) and np.array_equal(want.truth_count_sum, alone.truth_count_sum)


def test_slices_shards_accumulation_and_overwrite(hip_engine):
    import torch
    eng = hip_engine
    pool, tok, tr = pool_of(11, 100, 9, dist=4)
    nv, mk = pairs_for(100, 6, 9)
    want = shortest.shortest_prefix(pool, tok, tr, nv, mk, 3, 203, 11, M=101)
    dp, dt, dtr, dn, dm = to_dev(pool, tok, tr, nv, mk)
    out = eng.shortest_prefix_device(dp, dt, dtr, dn, dm, 3, 80, 11)                     # r slices add up
    kw = dict(tie_class_hits=out[0], voted_token_sum=out[1], spent_token_sum=out[2], latency_sum=out[3], truth_count_sum=out[4])
    eng.shortest_prefix_device(dp, dt, dtr, dn, dm, 80, 203, 11, **kw)
    per = torch.zeros((200, 6, 101), dtype=torch.int64, device=dp.device)
    for lo, hi in ((0, 4), (4, 11)):                                                     # p shards, each with its global offset
        eng.shortest_prefix_device(dp[lo:hi].contiguous(), dt[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dn, dm, 3, 203, 11, p_offset=lo,
                                   per_resample=per)
    eng.sync()
    assert_dev_same(out[:5] + (per, None, None), want)
    eng.shortest_prefix_device(dp, dt, dtr, dn, dm, 3, 203, 11, per_resample=per, **kw)  # DEVICE mode adds to what is there
    eng.sync()
    assert_dev_same(out[:5] + (per, None, None), want, times=2)
    whole = shortest.shortest_prefix(pool, tok, tr, nv, mk, want_cells=True)
    cells = torch.full((11, 6, 16), 0xAB, dtype=torch.uint8, device=dp.device)           # the cells are overwritten, the sums added to
    ctok = torch.full((11, 6), -7, dtype=torch.int64, device=dp.device)
    got = eng.shortest_prefix_device(dp, dt, dtr, dn, dm, cells=cells, cell_tokens=ctok)
    got = eng.shortest_prefix_device(dp, dt, dtr, dn, dm, cells=cells, cell_tokens=ctok, tie_class_hits=got[0], voted_token_sum=got[1],
                                     spent_token_sum=got[2], latency_sum=got[3], truth_count_sum=got[4])
    eng.sync()
    assert_dev_same(got, whole, per=False, times=2)
    raw = cells.cpu().numpy()
    assert np.array_equal(cells_from_torch(cells), whole.cells) and np.array_equal(ctok.cpu().numpy(), whole.cell_tokens)
    assert (raw[:, :, 13:] == 0xAB).all() or (raw[:, :, 13:] == 0).all()                 # (the record's padding is the kernel's to write or leave)
    for _ in range(2):                                                                   # HOST: the same answer twice, not twice the answer
        assert_host_same(eng.shortest_prefix(pool, tok, tr, nv, mk, want_cells=True), whole, per=False, cells=True)
    a = eng.shortest_prefix(pool[:4], tok[:4], tr[:4], nv, mk, want_cells=True)
    b = eng.shortest_prefix(pool[4:], tok[4:], tr[4:], nv, mk, want_cells=True)
    assert np.array_equal(a.spent_token_sum + b.spent_token_sum, whole.spent_token_sum)
    assert np.array_equal(np.concatenate([a.cells, b.cells]), whole.cells)


def test_one_graph_capture_and_replay():
    import torch
    pool, tok, tr = pool_of(20, 128, 33)
    nv, mk = pairs_for(128, 8, 33)
    want = shortest.shortest_prefix(pool, tok, tr, nv, mk, 0, 100, 4, M=129)
    dev = to_dev(pool, tok, tr, nv, mk)
    with Engine(device=0) as eng:                                       # no SCV_FLAG_TIMING: no event records in the graph
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros(s, dtype=torch.int64, device="cuda") for s in ((8, 1025), (8,), (8,), (8,), (8,), (100, 8, 129))]
        kw = dict(tie_class_hits=bufs[0], voted_token_sum=bufs[1], spent_token_sum=bufs[2], latency_sum=bufs[3], truth_count_sum=bufs[4],
                  per_resample=bufs[5])
        with torch.cuda.stream(side):                                   # warm-up on the capture stream
            eng.shortest_prefix_device(*dev, 0, 100, 4, **kw)
        torch.cuda.synchronize()
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.shortest_prefix_device(*dev, 0, 100, 4, **kw)
        g.replay()
        torch.cuda.synchronize()
        eng.sync()
        assert_dev_same(bufs + [None, None], want)


@pytest.mark.parametrize("N", [1, 8, 65, 128, 256])
def test_keeping_every_sample_is_the_resampled_vote(hip_engine, N):
    """m >= k against Engine.resample_prefix bit for bit; k = N gives the same cell for every ordering."""
    eng = hip_engine
    pool, tok, tr = pool_of(12, N, N, dist=1)
    rng = np.random.default_rng(N)
    nv = np.concatenate([[0, 1, N, N + 2], rng.integers(0, N + 1, size=6)]).astype(np.int32)
    mk = (nv + rng.integers(0, 3, size=nv.shape)).astype(np.int32)
    got = eng.shortest_prefix(pool, tok, tr, nv, mk, resamples=65, seed=3, r_begin=9, p_offset=4)
    ref = eng.resample_prefix(pool, tr, nv, 65, 3, tokens=tok, r_begin=9, p_offset=4, M=N + 1)
    assert np.array_equal(got.tie_class_hits, ref.tie_class_hits) and np.array_equal(got.per_resample, ref.per_resample)
    assert np.array_equal(got.truth_count_sum, ref.truth_count_sum)
    assert np.array_equal(got.voted_token_sum, ref.token_sum) and np.array_equal(got.spent_token_sum, ref.token_sum)
    from o1_inference_scaling_laws_amd.token_budget import orderings
    perm = orderings(12, N, 9, 74, 3, 4).reshape(12, 65, N)             # the latency is the largest token count of the prefix
    rows = np.arange(12)[:, None, None]
    for b, k in enumerate(np.clip(nv, 0, N)):
        assert int(got.latency_sum[b]) == (int(tok[rows, perm[:, :, :k]].max(axis=2).sum()) if k else 0), b
    full = np.full(4, N, dtype=np.int32)
    mk4 = np.array([1, max(N // 4, 1), max(N - 1, 1), N], dtype=np.int32)
    many = eng.shortest_prefix(pool, tok, tr, full, mk4, resamples=9, seed=5)
    one = eng.shortest_prefix(pool, tok, tr, full, mk4)
    assert (many.per_resample == many.per_resample[0]).all()
    for name in SUMS:
        assert np.array_equal(getattr(many, name), 9 * getattr(one, name)), name


def test_open_domain_equals_the_relabelled_pool(hip_engine):
    rng = np.random.default_rng(12)
    N = 70
    vals = np.unique(np.concatenate([rng.integers(-2 ** 31, 2 ** 31, size=9), [-2 ** 31, 2 ** 31 - 1, 0, 1023, 1024]])).astype(np.int64)
    idx = rng.integers(0, len(vals), size=(7, N))
    wide, small = vals[idx].astype(np.int32), idx.astype(np.int32)      # an order-preserving relabelling into 0 .. 13
    tr_i = rng.integers(0, len(vals), size=7)
    tok = rng.integers(0, 900, size=wide.shape).astype(np.int32)
    nv, mk = pairs_for(N, 8, 12)
    with Engine(device=0, open_domain=True) as oe:
        for R in (None, 67):
            want = both_modes(oe, wide, tok, vals[tr_i].astype(np.int32), nv, mk, 0, R, 6, open_domain=True)
            flag_off = hip_engine.shortest_prefix(small, tok, tr_i.astype(np.int32), nv, mk, resamples=R, seed=6, M=N + 1, want_cells=R is None)
            for name in SUMS:
                assert np.array_equal(getattr(flag_off, name), getattr(want, name)), name
            assert np.array_equal(flag_off.per_resample, want.per_resample)
            if R is None:
                # a relabelled row may not use every label: its codes are the ranks among the labels it does use
                code = np.array([[-1 if v < 0 else np.searchsorted(np.unique(small[p]), v) for v in flag_off.cells["min_mode"][p]] for p in range(7)])
                assert np.array_equal(code, want.cells["min_mode"]) and np.array_equal(flag_off.cells["max_count"], want.cells["max_count"])


def test_too_few_classes_is_an_error_at_sync(hip_engine):
    pool = np.tile(np.arange(8, dtype=np.int32), (3, 1))               # the whole pool is an 8-way tie
    tok = np.ones_like(pool)
    tr = np.array([0, 1, 2], dtype=np.int32)
    nv, mk = np.array([8], dtype=np.int32), np.array([8], dtype=np.int32)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.shortest_prefix(pool, tok, tr, nv, mk, resamples=5, M=8)
    assert ei.value.code == _lib.ERR_ARG
    out = hip_engine.shortest_prefix_device(*to_dev(pool, tok, tr, nv, mk), 0, 5, 1, M=4)
    with pytest.raises(_lib.ScvError) as ei:
        hip_engine.sync()
    assert ei.value.code == _lib.ERR_ARG
    assert int(out[0].cpu().numpy()[0, 8]) == 15                        # the tie-class table itself is complete
    hip_engine.sync()


def test_bad_arguments_are_refused_at_the_call(hip_engine):
    """every SCV_ERR_ARG case of the token-budget entry, and this entry's required pointers: nothing is queued, no output is touched."""
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 300), dtype=np.int32)
    tok = np.zeros((2, 300), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nv = np.ones(40, dtype=np.int32)
    tie = np.full((40, 1025), -1, dtype=np.int64)
    sums = np.full(40, -1, dtype=np.int64)
    cells = np.full(600 * 16, 0xCD, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(N=8, B=2, order=1, r0=0, r1=4, p_off=0, M=1, per=None, nvp=nv, mkp=nv, tiep=tie, tokp=tok, poolp=pool, trp=tr, c=None, ct=None,
             mem=_lib.MEM_HOST):
        return L.scv_shortest_prefix_i32(ctx, ptr(poolp), ptr(tokp), ptr(nvp), ptr(mkp), ptr(trp), 2, B, N, p_off, order, r0, r1, 1, M, mem,
                                         ptr(tiep), ptr(sums), ptr(sums), ptr(sums), ptr(sums), ptr(per), ptr(c), ptr(ct))
    hip_engine.sync()
    hip_engine.drain_kernel_ns()                                        # (the session engine times its launches: a queued kernel would count)
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=33), dict(order=2), dict(order=-1), dict(order=0), dict(order=0, r0=1, r1=2),
               dict(order=0, r0=0, r1=0), dict(c=cells), dict(ct=sums), dict(r0=5, r1=4), dict(r0=-1), dict(p_off=-1),
               dict(per=np.zeros((4, 2, 1), dtype=np.int64), M=0), dict(nvp=None), dict(mkp=None), dict(tiep=None), dict(tokp=None),
               dict(poolp=None), dict(trp=None), dict(mem=7)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"shortest" in L.scv_last_error() or kw == dict(mem=7), kw
        assert (tie == -1).all() and (sums == -1).all() and (cells == 0xCD).all(), kw
    hip_engine.sync()                                                   # nothing was queued: no error word to report
    assert hip_engine.drain_kernel_ns()[1] == 0
    assert call() == _lib.OK and not (tie[:2] == -1).any()
    assert hip_engine.drain_kernel_ns()[1] == 1
    assert call(order=0, r0=0, r1=1, c=cells, ct=sums) == _lib.OK


def test_the_curve_records(hip_engine):
    P, N, R = 30, 128, 200
    pool, tok, tr = pool_of(P, N, 2025)
    pairs = [(k, m) for k in (1, 2, 4, 8, 16, 32, 64, 128) for m in sorted({1, (k + 3) // 4, k})]
    recs = curves.shortest_vote_records(hip_engine, pool, tr, tok, pairs, resamples=R, seed=17)
    want = shortest.shortest_prefix(pool, tok, tr, [k for k, _ in pairs], [m for _, m in pairs], 0, R, 17)
    assert [(r["k"], r["m"]) for r in recs] == pairs
    assert [r["accuracy"] for r in recs] == [want.accuracy(b) for b in range(len(pairs))]
    assert [r["avg_tokens_used"] for r in recs] == [float(want.avg_spent_tokens(b)) for b in range(len(pairs))]
    assert [r["avg_latency"] for r in recs] == [float(want.avg_latency(b)) for b in range(len(pairs))]
    assert all(r["avg_voted_tokens"] <= r["avg_tokens_used"] <= r["k"] * r["avg_latency"] for r in recs)


def test_fuzz(hip_engine):
    """100 random draws of shape, order, budgets, token kind, slice and shard."""
    rng = np.random.default_rng(20261020)
    for draw in range(100):
        N = int(rng.choice([1, 2, 3, 7, 31, 32, 33, 64, 65, 100, 129, 200, 256]))
        shuffled = bool(rng.integers(0, 2))
        P = int(rng.integers(1, 9)) if shuffled else int(rng.integers(1, 80))
        R = int(rng.choice([1, 2, 9, 64, 70])) if shuffled else None
        B = int(rng.choice([1, 2, 7, 32]))
        pool, tok, tr = pool_of(P, N, 7000 + draw, dist=draw % 6, tokens=("synth", "two", "equal", "zeros")[int(rng.integers(0, 4))])
        nv, mk = pairs_for(N, B, draw)
        r0 = int(rng.integers(0, 1000)) if shuffled else 0
        p_off = int(rng.choice([0, 3, 1 << 35]))
        seed = int(rng.integers(0, 2 ** 63))
        M = N + 1
        want = shortest.shortest_prefix(pool, tok, tr, nv, mk, r0, r0 + R if shuffled else None, seed, p_off, M=M, want_cells=not shuffled)
        if draw % 2:
            got = hip_engine.shortest_prefix_device(*to_dev(pool, tok, tr, nv, mk), r0, r0 + R if shuffled else None, seed, p_offset=p_off, M=M,
                                                    want_cells=not shuffled)
            hip_engine.sync()
            assert_dev_same(got, want, cells=not shuffled)
        else:
            host = hip_engine.shortest_prefix(pool, tok, tr, nv, mk, resamples=R, seed=seed, r_begin=r0, p_offset=p_off, M=M,
                                              want_cells=not shuffled)
            assert_host_same(host, want, cells=not shuffled)
