"""GPU tests of the HOST-mode staging of the lane-body entries (scv_resample_prefix_i32, scv_token_budget_prefix_i32,
scv_weighted_prefix_i32, scv_adaptive_prefix_i32) where the per-entry suites leave it open: a shuffled call of two chunks (per_resample and
every sum accumulate over the chunks, each chunk launched with its own p_offset), a pool-order call of two chunks with the optional regions
absent (no tokens, no rule flags), empty calls with no ordering drawn, and scv_resample_prefix_i32 through the pinned small block and through
the staging buffer.  Every HOST result is compared bit for bit with ONE DEVICE launch over the same inputs; the DEVICE path is held to the CPU
mirrors by the per-entry suites."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, adaptive, synth, weighted
from o1_inference_scaling_laws_amd.engine import cells_from_torch

pytestmark = pytest.mark.gpu

N, B = 256, 32
R0, R, M, SEED = 5, 2, N + 1, 77          # two orderings from r_begin = 5, per_resample with N + 1 classes
CHUNK_BYTES = 64 << 20                     # a chunk is 64 MiB / (bytes per problem) problems


def to_dev(*arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def host(x):
    return None if x is None else x.cpu().numpy()


@pytest.fixture(scope="module")
def data():
    """65 600 pools of 256 votes with tokens, truth, weights and 32 budgets / rules: every test takes the first P rows.  Read only."""
    a, t, tr = synth.fill(65_600, 1, N, 31, 1, want_tokens=True)
    pool, tok = np.ascontiguousarray(a[:, 0, :]), np.ascontiguousarray(t[:, 0, :])
    w = (1 + (tok % 1000)).astype(np.int32)
    nv = np.arange(8, 264, 8, dtype=np.int32)
    bud = np.array([2 ** 11 * k for k in range(1, 33)], dtype=np.int64) * 16
    rng = np.random.default_rng(31)
    built = [adaptive.never(N), adaptive.margin_rule(N, 1), adaptive.margin_rule(N, 3), adaptive.beta_rule(N, 0.9)]
    cap = rng.choice([0, 1, N // 2, N, N + 7], size=B).astype(np.int32)
    need = np.stack([built[b % len(built)] for b in range(B)]).astype(np.int32)
    flags = rng.integers(0, 2, size=B).astype(np.int32)
    for x in (pool, tok, tr, w, nv, bud, cap, need, flags):
        x.setflags(write=False)
    return dict(pool=pool, tok=tok, tr=tr, w=w, nv=nv, bud=bud, cap=cap, need=need, flags=flags)


def test_token_budget_shuffled_two_chunks(hip_engine, data):
    P = 33_000                              # no cells: 64 MiB / (2 * 256 * 4 + 4) = 32 704 pools per chunk
    assert CHUNK_BYTES // (2 * N * 4 + 4) == 32_704 < P
    pool, tok, tr, bud = data["pool"][:P], data["tok"][:P], data["tr"][:P], data["bud"]
    got = hip_engine.token_budget_prefix(pool, tok, tr, bud, resamples=R, seed=SEED, r_begin=R0, M=M)
    dev = hip_engine.token_budget_prefix_device(*to_dev(pool, tok, tr, bud), r_begin=R0, r_end=R0 + R, seed=SEED, M=M)
    hip_engine.sync()
    tie, ts, vs, tcs, per = [host(x) for x in dev[:5]]
    assert per.shape == (R, B, M) and per.any()
    assert np.array_equal(got.tie_class_hits, tie) and np.array_equal(got.token_sum, ts) and np.array_equal(got.vote_count_sum, vs)
    assert np.array_equal(got.truth_count_sum, tcs) and np.array_equal(got.per_resample, per)


@pytest.mark.parametrize("with_tokens", [True, False])
def test_weighted_shuffled_two_chunks(hip_engine, data, with_tokens):
    # no cells, with tokens: 64 MiB / (3 * 256 * 4 + 4) = 21 816 pools per chunk; without: 64 MiB / (2 * 256 * 4 + 4) = 32 704
    P, chunk = (22_000, 21_816) if with_tokens else (33_000, 32_704)
    assert CHUNK_BYTES // ((3 if with_tokens else 2) * N * 4 + 4) == chunk < P
    pool, w, tr, nv = data["pool"][:P], data["w"][:P], data["tr"][:P], data["nv"]
    tok = data["tok"][:P] if with_tokens else None
    got = hip_engine.weighted_prefix(pool, w, tr, nv, 0, resamples=R, seed=SEED, r_begin=R0, M=M, tokens=tok)
    dev = hip_engine.weighted_prefix_device(*to_dev(pool, w, tr, nv), 0, r_begin=R0, r_end=R0 + R, seed=SEED, tokens=to_dev(tok)[0], M=M)
    hip_engine.sync()
    tie, ts, per = [host(x) for x in dev[:3]]
    assert per.shape == (R, B, M) and per.any()
    assert np.array_equal(got.tie_class_hits, tie) and np.array_equal(got.per_resample, per)
    assert (ts is None and got.token_sum is None) if not with_tokens else np.array_equal(got.token_sum, ts)


@pytest.mark.parametrize("with_tokens", [True, False])
def test_adaptive_shuffled_two_chunks(hip_engine, data, with_tokens):
    # no cells, with tokens: 64 MiB / (2 * 256 * 4 + 4) = 32 704 pools per chunk; without: 64 MiB / (256 * 4 + 4) = 65 280
    P, chunk = (33_000, 32_704) if with_tokens else (65_600, 65_280)
    assert CHUNK_BYTES // ((2 if with_tokens else 1) * N * 4 + 4) == chunk < P
    pool, tr, cap, need, flags = data["pool"][:P], data["tr"][:P], data["cap"], data["need"], data["flags"]
    tok = data["tok"][:P] if with_tokens else None
    got = hip_engine.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, resamples=R, seed=SEED, r_begin=R0, M=M)
    dev = hip_engine.adaptive_prefix_device(*to_dev(pool, tr, cap, need, flags), tokens=to_dev(tok)[0], r_begin=R0, r_end=R0 + R, seed=SEED, M=M)
    hip_engine.sync()
    tie, ts, vs, tcs, hist, per = [host(x) for x in dev[:6]]
    assert per.shape == (R, B, M) and per.any() and hist.any()
    assert np.array_equal(got.tie_class_hits, tie) and np.array_equal(got.vote_count_sum, vs) and np.array_equal(got.truth_count_sum, tcs)
    assert np.array_equal(got.stop_hist, hist) and np.array_equal(got.per_resample, per)
    assert (ts is None and got.token_sum is None) if not with_tokens else np.array_equal(got.token_sum, ts)


def test_weighted_pool_order_without_tokens_two_chunks(hip_engine, data):
    P = 26_400                              # cells, no tokens, no cell tokens: 64 MiB / (2 * 256 * 4 + 4 + 32 * 16) = 26 173 pools per chunk
    assert CHUNK_BYTES // (2 * N * 4 + 4 + B * 16) == 26_173 < P
    pool, w, tr, nv = data["pool"][:P], data["w"][:P], data["tr"][:P], data["nv"]
    got = hip_engine.weighted_prefix(pool, w, tr, nv, 0, tokens=None, want_cells=True, M=0)
    dev = hip_engine.weighted_prefix_device(*to_dev(pool, w, tr, nv), 0, want_cells=True)
    hip_engine.sync()
    assert got.token_sum is None and got.cell_tokens is None and dev[1] is None and dev[4] is None
    assert np.array_equal(got.tie_class_hits, host(dev[0])) and np.array_equal(got.cells, cells_from_torch(dev[3]))
    sample = [0, 26_172, 26_173, P - 1]
    want = weighted.weighted_prefix(pool[sample], w[sample], tr[sample], nv, 0, want_cells=True)
    assert np.array_equal(got.cells[sample], want.cells)


def test_adaptive_pool_order_without_tokens_and_flags_two_chunks(hip_engine, data):
    P = 40_500                              # cells and cell votes, no tokens: 64 MiB / (256 * 4 + 4 + 32 * (16 + 4)) = 40 233 pools per chunk
    assert CHUNK_BYTES // (N * 4 + 4 + B * (16 + 4)) == 40_233 < P
    pool, tr, cap, need = data["pool"][:P], data["tr"][:P], data["cap"], data["need"]
    got = hip_engine.adaptive_prefix(pool, tr, cap, need, None, tokens=None, want_cells=True, M=0)
    dev = hip_engine.adaptive_prefix_device(*to_dev(pool, tr, cap, need), None, want_cells=True)
    hip_engine.sync()
    assert got.token_sum is None and got.cell_tokens is None and dev[1] is None and dev[7] is None
    assert np.array_equal(got.tie_class_hits, host(dev[0])) and np.array_equal(got.stop_hist, host(dev[4]))
    assert np.array_equal(got.vote_count_sum, host(dev[2])) and np.array_equal(got.truth_count_sum, host(dev[3]))
    assert np.array_equal(got.cells, cells_from_torch(dev[6])) and np.array_equal(got.cell_votes, host(dev[8]))
    sample = [0, 40_232, 40_233, P - 1]
    want = adaptive.adaptive_prefix(pool[sample], tr[sample], cap, need, None, want_cells=True)
    assert np.array_equal(got.cells[sample], want.cells) and np.array_equal(got.cell_votes[sample], want.cell_votes)


def test_host_calls_that_draw_no_ordering_zero_every_output(hip_engine):
    """P > 0 with an empty range of r, for the entries whose own suites make only the P = 0 call (test_gpu_weighted.py makes both)."""
    L, ctx = _lib.load(), hip_engine._ctx
    pool = np.zeros((2, 8), dtype=np.int32)
    tr = np.zeros(2, dtype=np.int32)
    nv = np.ones(2, dtype=np.int32)
    bud = np.ones(2, dtype=np.int64)
    need = np.ones((2, 9), dtype=np.int32)
    tie = np.full((2, 1025), -1, dtype=np.int64)
    tok, votes, tcs = (np.full(2, -1, dtype=np.int64) for _ in range(3))
    hist = np.full((2, 9), -1, dtype=np.int64)
    per = np.full((0, 2, 4), -1, dtype=np.int64)
    outs = (tie, tok, votes, tcs, hist)
    ptr = lambda a: a.ctypes.data  # noqa: E731

    def refill():
        for x in outs:
            x[:] = -1
    assert L.scv_resample_prefix_i32(ctx, ptr(pool), ptr(pool), ptr(nv), ptr(tr), 2, 2, 8, 0, 5, 5, 1, 4, _lib.MEM_HOST, ptr(tie), ptr(tok),
                                     ptr(tcs), ptr(per)) == _lib.OK
    assert not tie.any() and not tok.any() and not tcs.any()
    refill()
    assert L.scv_token_budget_prefix_i32(ctx, ptr(pool), ptr(pool), ptr(bud), ptr(tr), 2, 2, 8, 0, _lib.ORDER_SHUFFLED, 5, 5, 1, 4,
                                         _lib.MEM_HOST, ptr(tie), ptr(tok), ptr(votes), ptr(tcs), ptr(per), None, None) == _lib.OK
    assert not tie.any() and not tok.any() and not votes.any() and not tcs.any()
    refill()
    assert L.scv_adaptive_prefix_i32(ctx, ptr(pool), ptr(pool), ptr(nv), ptr(need), None, ptr(tr), 2, 2, 8, 0, _lib.ORDER_SHUFFLED, 5, 5, 1, 4,
                                     _lib.MEM_HOST, ptr(tie), ptr(tok), ptr(votes), ptr(tcs), ptr(hist), ptr(per), None, None, None) == _lib.OK
    assert not any(x.any() for x in outs)
    refill()                                                            # ... and P = 0 with a token sum, which test_gpu_adaptive.py passes as NULL
    assert L.scv_adaptive_prefix_i32(ctx, None, None, ptr(nv), ptr(need), None, None, 0, 2, 8, 0, _lib.ORDER_SHUFFLED, 0, 3, 1, 4,
                                     _lib.MEM_HOST, ptr(tie), None, ptr(votes), ptr(tcs), ptr(hist), None, None, None, None) == _lib.OK
    assert not tie.any() and not votes.any() and not tcs.any() and not hist.any() and (tok == -1).all()


def test_resample_small_block_and_staging_buffer_agree(hip_engine, data):
    eng = hip_engine
    P, n = 40, 64
    pool, tok, tr = np.ascontiguousarray(data["pool"][:P, :n]), np.ascontiguousarray(data["tok"][:P, :n]), data["tr"][:P]
    nv = np.array([1, 2, 7, 64], dtype=np.int32)
    res = []
    try:
        for kb in (1024, 0):                # the default (this call is ~60 KiB: the pinned small block), then never small
            eng.set_option("host_small_kb", kb)
            n0 = eng.stat("resample_calls")
            res.append(eng.resample_prefix(pool, tr, nv, 9, SEED, tokens=tok, r_begin=R0))
            assert eng.stat("resample_calls") == n0 + 1
    finally:
        eng.set_option("host_small_kb", 1024)
    a, b = res
    assert a.tie_class_hits.any() and a.per_resample.any()
    for f in ("tie_class_hits", "token_sum", "truth_count_sum", "per_resample"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
