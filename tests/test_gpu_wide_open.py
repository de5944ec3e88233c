"""GPU tests of scv_resample_wide_i32 on SCV_FLAG_OPEN_DOMAIN contexts (any int32 answer in pools of up to 4096 samples): every output
bit-exact against the CPU mirror (o1_inference_scaling_laws_amd/wide.py, open_domain=True) over the value classes of a row (all equal, all
distinct, D = 2, D around 1024, D = N = 4096, both ends of int32, the truth absent / smallest / largest), the relabelling identity against a
flag-off context, no change on pools inside 0..1023, problems of different D inside one workgroup's run, tie classes beyond the table, the
clamp flag, accumulation / overwrite, slices and shards, a fresh context, a captured graph, and 100 random draws."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, wide
from tests.test_gpu_resample import budgets_for
from tests.test_gpu_wide import NS, RS, pool_of, to_dev
from tests.test_wide_open_cpu import relabel_wide, truth_for, wide_pool, wide_row

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def open_engine():
    from o1_inference_scaling_laws_amd.engine import Engine
    with Engine(device=0, open_domain=True) as eng:
        yield eng


def tokens_for(rng, pool, tokens):
    return rng.integers(0, 5000, size=pool.shape).astype(np.int32) if tokens else None


def check(got, want, tokens, M, what=None, times=1):
    """got: (tie, token_sum, truth_count_sum, per_resample) as numpy arrays or device tensors."""
    tie, tok, tcs, per = [x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy() for x in got]
    assert np.array_equal(tie, times * want.tie_class_hits), what
    assert np.array_equal(tcs, times * want.truth_count_sum), what
    if tokens:
        assert np.array_equal(tok, times * want.token_sum), what
    if M:
        assert np.array_equal(per, times * want.per_resample), what


def sync_expecting(eng, error_bits):
    """The mirror's error bits decide: bit 1 (a hit with n_modes >= M or >= 1025) is SCV_ERR_ARG at scv_sync, and the word is cleared."""
    if error_bits:
        with pytest.raises(_lib.ScvError) as ei:
            eng.sync()
        assert ei.value.code == _lib.ERR_ARG
    eng.sync()


def host_result(res):
    return res.tie_class_hits, res.token_sum, res.truth_count_sum, res.per_resample


def test_negative_edge_and_hash_values_succeed_and_equal_the_mirror(open_engine):
    """Fails without the feature: the wide entry answered SCV_ERR_DOMAIN for these pools with the flag on or off."""
    eng = open_engine
    rng = np.random.default_rng(1)
    N = 700
    pool, tr = wide_pool(rng, N, ["hash", "edges", "bitpairs", "mixed", "hash"], truths=("modal", "smallest", "present", "largest", "absent"))
    pool[0, :3] = (-1, -2 ** 31, 2 ** 31 - 1)
    assert (pool < 0).any() and (pool > 1023).any()
    tok = tokens_for(rng, pool, True)
    nv = np.array([1, 2, 4, 64, 699, 700, 0], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 3, 12, seed=77, tokens=tok, p_offset=2, M=701, open_domain=True)
    assert want.error_bits == 0 and want.tie_class_hits.sum() > 0
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    got = eng.resample_wide_device(dp, dtr, dnv, 3, 12, 77, tokens=dt, p_offset=2, M=701)
    eng.sync()
    check(got, want, True, 701)
    res = eng.resample_wide(pool, tr, nv, 9, 77, tokens=tok, r_begin=3, p_offset=2, M=701)
    check(host_result(res), want, True, 701)


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_mirror(open_engine, N, tokens):
    eng = open_engine
    k = NS.index(N) + (1 if tokens else 0)
    rng = np.random.default_rng(6000 + 2 * N + tokens)
    classes = ["distinct", "two", "edges", "equal"] + (["d1023", "d1024", "d1025"] if N >= 1025 else ["hash", "mixed", "special"])
    pool, tr = wide_pool(rng, N, classes, shift=k)                          # truths: absent, smallest, largest, present, modal from k on
    tok = tokens_for(rng, pool, tokens)
    R = RS[k % len(RS)]
    r0 = (0, 7, 2 ** 31 - 1 - R)[k % 3]
    p_off = (0, 5, 1 << 33)[(k + 1) % 3]
    nv = np.array(budgets_for(N, k % 3), dtype=np.int32)
    M = int(np.clip(nv, 0, N).max()) + 1
    want = wide.resample_wide(pool, tr, nv, r0, r0 + R, seed=11 + k, tokens=tok, p_offset=p_off, M=M, open_domain=True)
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    got = eng.resample_wide_device(dp, dtr, dnv, r0, r0 + R, 11 + k, tokens=dt, p_offset=p_off, M=M)
    sync_expecting(eng, want.error_bits)                                    # (N >= 1025, all distinct, a large budget: classes beyond the table)
    check(got, want, tokens, M)


@pytest.mark.parametrize("N", [64, 1024, 2048])
def test_flag_on_equals_a_flag_off_context_on_the_relabelled_pool(open_engine, hip_engine, N):
    rng = np.random.default_rng(70 + N)
    classes = ["equal", "two", "edges", "special"] + (["hash", "distinct"] if N <= 1024 else ["d1023", "d1024"])    # D <= 1024 in every row
    pool, tr = wide_pool(rng, N, classes, shift=N)
    enc, tcode = relabel_wide(pool, tr)
    tok = tokens_for(rng, pool, True)
    nv = np.array([1, 3, N // 2, N - 1, N], dtype=np.int32)
    outs = []
    for eng, (pl, t) in ((open_engine, (pool, tr)), (hip_engine, (enc, tcode))):
        dp, dt, dtr, dnv = to_dev(pl, tok, t, nv)
        got = eng.resample_wide_device(dp, dtr, dnv, 5, 38, 9, tokens=dt, p_offset=3, M=N + 1)
        eng.sync()
        outs.append([x.cpu().numpy() for x in got])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert outs[0][0].sum() > 0


@pytest.mark.parametrize("dist", range(6))
def test_pools_inside_the_bins_are_unchanged_by_the_flag(open_engine, hip_engine, dist):
    N = (700, 1500, 64, 1024, 2049, 300)[dist]
    pool, tok, tr = pool_of(5, N, 90 + dist, dist, True)
    nv = np.array(budgets_for(N, dist % 3), dtype=np.int32)
    M = int(np.clip(nv, 0, N).max()) + 1
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    outs = []
    for eng in (open_engine, hip_engine):
        got = eng.resample_wide_device(dp, dtr, dnv, 0, 21, 31, tokens=dt, M=M)
        eng.sync()
        outs.append([x.cpu().numpy() for x in got])
        res = eng.resample_wide(pool, tr, nv, 21, 31, tokens=tok, M=M)
        for a, b in zip(outs[-1], host_result(res)):
            assert np.array_equal(a, b)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("grid", [1, 2])
def test_problems_of_different_D_inside_one_run(grid, reverse):
    """Rows of 2000, 3, 900 and 1 distinct values walked by one or two workgroups: a bin, a truth code or a D left from the last problem
    would show."""
    from o1_inference_scaling_laws_amd.engine import Engine
    N, R = 2048, 5
    rng = np.random.default_rng(5)
    rows = [wide_row(rng, N, c) for c in ("d2000", "d3", "d900", "d1")]
    kinds = ("largest", "absent", "modal", "present")                      # the largest code of 2000 values, then a row without the truth
    truth = [truth_for(rng, r, kind) for r, kind in zip(rows, kinds)]
    if reverse:
        rows, truth = rows[::-1], truth[::-1]
    pool, tr = np.stack(rows).astype(np.int32), np.array(truth, dtype=np.int64).astype(np.int32)
    tok = tokens_for(rng, pool, True)
    nv = np.array([0, 1, N, 2, 1000, 1024, 1025, 2047], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 1, 1 + R, seed=6, tokens=tok, M=N + 1, open_domain=True)
    assert want.error_bits == 0
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    with Engine(device=0, open_domain=True) as eng:
        eng.set_option("grid", grid)
        got = eng.resample_wide_device(dp, dtr, dnv, 1, 1 + R, 6, tokens=dt, M=N + 1)
        eng.sync()
        check(got, want, True, N + 1)
        res = eng.resample_wide(pool, tr, nv, R, 6, tokens=tok, r_begin=1, M=N + 1)
        check(host_result(res), want, True, N + 1)


def test_tie_classes_beyond_the_table(open_engine):
    eng = open_engine
    N, R = 1025, 4
    row = wide_row(np.random.default_rng(1), N, "distinct")
    pool = row[None, :].astype(np.int32)
    tr = np.array([row[17]], dtype=np.int64).astype(np.int32)
    absent = np.array([truth_for(np.random.default_rng(2), row, "absent")], dtype=np.int64).astype(np.int32)
    M = 1100
    # budget 1024: a 1024-way tie lands in the last column, no error
    nv = np.array([1024], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 0, R, seed=4, M=M, open_domain=True)
    assert want.error_bits == 0 and want.tie_class_hits[0, 1024] > 0
    dp, dtr, dab, dnv = to_dev(pool, tr, absent, nv)
    got = eng.resample_wide_device(dp, dtr, dnv, 0, R, 4, M=M)
    eng.sync()
    check(got, want, False, M)
    check(host_result(eng.resample_wide(pool, tr, nv, R, 4, M=M)), want, False, M)
    # budget 1025: n_modes = 1025 has no column -- SCV_ERR_ARG, the hit counted nowhere, the truth count still added
    nv2 = np.array([1024, 1025], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv2, 0, R, seed=4, M=M, open_domain=True)
    assert want.error_bits == 2 and want.tie_class_hits[1].sum() == 0 and want.truth_count_sum[1] == R
    dnv2, = to_dev(nv2)
    got = eng.resample_wide_device(dp, dtr, dnv2, 0, R, 4, M=M)
    sync_expecting(eng, 2)
    check(got, want, False, M)
    with pytest.raises(_lib.ScvError) as ei:
        eng.resample_wide(pool, tr, nv2, R, 4, M=M)
    assert ei.value.code == _lib.ERR_ARG
    # the truth absent: nothing hits, no error
    want = wide.resample_wide(pool, absent, nv2, 0, R, seed=4, M=M, open_domain=True)
    assert want.error_bits == 0
    got = eng.resample_wide_device(dp, dab, dnv2, 0, R, 4, M=M)
    eng.sync()
    check(got, want, False, M)
    check(host_result(eng.resample_wide(pool, absent, nv2, R, 4, M=M)), want, False, M)


def test_the_clamp_flag_changes_nothing_under_the_open_flag():
    from o1_inference_scaling_laws_amd.engine import Engine
    rng = np.random.default_rng(8)
    pool, tr = wide_pool(rng, 1300, ["hash", "edges", "d1025", "two"], shift=2)
    tok = tokens_for(rng, pool, True)
    nv = np.array([1, 7, 650, 1024], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 0, 6, seed=2, tokens=tok, M=1025, open_domain=True)
    assert want.error_bits == 0
    with Engine(device=0, open_domain=True, clamp_to_invalid_bin=True) as eng:
        check(host_result(eng.resample_wide(pool, tr, nv, 6, 2, tokens=tok, M=1025)), want, True, 1025)
        dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
        got = eng.resample_wide_device(dp, dtr, dnv, 0, 6, 2, tokens=dt, M=1025)
        eng.sync()
        check(got, want, True, 1025)


def test_host_overwrites_device_accumulates_slices_and_shards_add_up(open_engine):
    import torch
    eng = open_engine
    rng = np.random.default_rng(12)
    N, R, M = 1100, 30, 1101
    pool, tr = wide_pool(rng, N, ["hash", "d1025", "edges", "mixed", "two", "equal", "d1023"], shift=1)
    tok = tokens_for(rng, pool, True)
    nv = np.array([N, 1, 64, 7, 300, 1024], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 3, 3 + R, seed=5, tokens=tok, M=M, open_domain=True)
    assert want.error_bits == 0
    for small_kb in (0, None, None):                                        # both HOST paths; the same answer again, not twice the answer
        if small_kb is not None:
            eng.set_option("host_small_kb", small_kb)
        try:
            check(host_result(eng.resample_wide(pool, tr, nv, R, 5, tokens=tok, r_begin=3, M=M)), want, True, M)
        finally:
            if small_kb is not None:
                eng.set_option("host_small_kb", 1024)                    # the default
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    bufs = eng.resample_wide_device(dp, dtr, dnv, 3, 3 + R, 5, tokens=dt, M=M)
    eng.resample_wide_device(dp, dtr, dnv, 3, 3 + R, 5, tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2],
                             per_resample=bufs[3])
    eng.sync()
    check(bufs, want, True, M, times=2)
    tie, ts, tcs, _ = eng.resample_wide_device(dp, dtr, dnv, 3, 14, 5, tokens=dt)                      # slices of r
    eng.resample_wide_device(dp, dtr, dnv, 14, 3 + R, 5, tokens=dt, tie_class_hits=tie, token_sum=ts, truth_count_sum=tcs)
    per = torch.zeros((R, len(nv), M), dtype=torch.int64, device=dp.device)
    for lo, hi in ((0, 3), (3, 7)):                                                                    # shards of p, each with its offset
        eng.resample_wide_device(dp[lo:hi].contiguous(), dtr[lo:hi].contiguous(), dnv, 3, 3 + R, 5, tokens=dt[lo:hi].contiguous(),
                                 p_offset=lo, per_resample=per)
    eng.sync()
    check((tie, ts, tcs, per), want, True, M)


def test_first_call_of_a_fresh_context_and_a_captured_graph():
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    rng = np.random.default_rng(13)
    N, R, M = 1500, 20, 1501
    pool, tr = wide_pool(rng, N, ["hash", "d1025", "edges", "two", "d40"], shift=3)
    tok = tokens_for(rng, pool, True)
    nv = np.array([1 << k for k in range(11)] + [N], dtype=np.int32)
    want = wide.resample_wide(pool, tr, nv, 0, R, seed=4, tokens=tok, M=M, open_domain=True)
    assert want.error_bits == 0
    dp, dt, dtr, dnv = to_dev(pool, tok, tr, nv)
    with Engine(device=0, open_domain=True) as eng:                        # no SCV_FLAG_TIMING: no event records in the graph
        got = eng.resample_wide_device(dp, dtr, dnv, 0, R, 4, tokens=dt, M=M)
        eng.sync()
        check(got, want, True, M)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        bufs = [torch.zeros_like(x) for x in got]
        kw = dict(tokens=dt, tie_class_hits=bufs[0], token_sum=bufs[1], truth_count_sum=bufs[2], per_resample=bufs[3])
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
            eng.resample_wide_device(dp, dtr, dnv, 0, R, 4, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            eng.resample_wide_device(dp, dtr, dnv, 0, R, 4, **kw)
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g.replay()
        g.replay()                                                         # replayed twice: DEVICE mode accumulates
        torch.cuda.synchronize()
        eng.sync()
        check(bufs, want, True, M, times=2)


FUZZ_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1100, 2047, 2048, 2049, 4095, 4096)
FUZZ_CLASSES = ("equal", "distinct", "two", "edges", "hash", "mixed", "special", "bitpairs", "few")


def fuzz_draw(seed):
    """One valid call that depends on the seed alone (P * R * N <= 300 000)."""
    rng = np.random.default_rng((9_100_000, seed))
    N = int(rng.choice(FUZZ_N)) if rng.random() < 0.6 else int(rng.integers(1, 1400))
    B = int(rng.choice((1, 2, 31, 32))) if rng.random() < 0.3 else int(rng.integers(1, 12))
    R = int(rng.choice((1, 2, 3, 64, 65))) if rng.random() < 0.4 else int(rng.integers(1, 30))
    P = int(rng.integers(1, 7))
    while P * R * N > 300_000 and R > 1:
        R = max(1, R // 2)
    pal = list(FUZZ_CLASSES) + [f"d{d}" for d in (1023, 1024, 1025, 40) if d <= N]
    classes = [pal[int(rng.integers(0, len(pal)))] for _ in range(P)]
    pool, tr = wide_pool(rng, N, classes, shift=int(rng.integers(0, 5)))
    tok = tokens_for(rng, pool, bool(rng.random() < 0.6))
    edges = [-3, 0, 1, N - 1, N, N + 1, 1024, 1025]
    nv = np.array([int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(0, N + 2)) for _ in range(B)], dtype=np.int32)
    kmax = int(np.clip(nv, 0, N).max())
    M = None if rng.random() < 0.3 else (kmax + 1 if rng.random() < 0.8 else max(1, kmax // 2))
    return dict(P=P, N=N, B=B, R=R, classes=classes, pool=pool, tok=tok, tr=tr, nv=nv, r0=int(rng.choice((0, 7, 2 ** 31 - 1 - R))),
                p_off=int(rng.choice((0, 5, 1 << 33))), seed=int(rng.integers(0, 2 ** 63)), M=M, device=bool(rng.random() < 0.5),
                grid=(int(rng.integers(1, 9)) if rng.random() < 0.4 else 0))


@pytest.mark.parametrize("part", range(4))
def test_fuzz_100_draws(part):
    from o1_inference_scaling_laws_amd.engine import Engine
    with Engine(device=0, open_domain=True) as eng:
        for seed in range(25 * part, 25 * part + 25):
            c = fuzz_draw(seed)
            want = wide.resample_wide(c["pool"], c["tr"], c["nv"], c["r0"], c["r0"] + c["R"], seed=c["seed"], tokens=c["tok"],
                                      p_offset=c["p_off"], M=c["M"], open_domain=True)
            eng.set_option("grid", c["grid"])
            what = {k: v for k, v in c.items() if k not in ("pool", "tok", "tr")}
            if c["device"]:
                dp, dt, dtr, dnv = to_dev(c["pool"], c["tok"], c["tr"], c["nv"])
                got = eng.resample_wide_device(dp, dtr, dnv, c["r0"], c["r0"] + c["R"], c["seed"], tokens=dt, p_offset=c["p_off"], M=c["M"])
                sync_expecting(eng, want.error_bits)
                check(got, want, c["tok"] is not None, c["M"], what)
            elif want.error_bits:
                with pytest.raises(_lib.ScvError) as ei:
                    eng.resample_wide(c["pool"], c["tr"], c["nv"], c["R"], c["seed"], tokens=c["tok"], r_begin=c["r0"], p_offset=c["p_off"],
                                      M=c["M"] or 0)
                assert ei.value.code == _lib.ERR_ARG, what
            else:
                res = eng.resample_wide(c["pool"], c["tr"], c["nv"], c["R"], c["seed"], tokens=c["tok"], r_begin=c["r0"], p_offset=c["p_off"],
                                        M=c["M"] or 0)
                check(host_result(res), want, c["tok"] is not None, c["M"], what)
