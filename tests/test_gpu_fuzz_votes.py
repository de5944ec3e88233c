"""Randomised parity of the ordering, draw and exact votes: 120 seeded calls of each lane body of scv_resample_prefix (resample, token budget,
weighted, adaptive, draws with replacement), every output bit for bit against its numpy mirror; 60 calls of the exact expected vote within
1e-12 of the rationals; 40 sequences of 12 calls that mix all eight entries, both modes and the grid option on ONE context; a count of 65535.
The draws are tests/_vote_fuzz.py (what they reach and that they discriminate: tests/test_vote_fuzz_cpu.py).

Work bound of one call: P * R * (largest budget, or N) <= 1.5e6 (adaptive: 3e5), a fifth of that inside a sequence (_vote_fuzz.WORK).
SCV_FUZZ_VOTE_SEEDS / SCV_FUZZ_EXPECTED_SEEDS / SCV_FUZZ_MIXED_SEEDS and SCV_FUZZ_FIRST move the seed ranges."""
import os

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, expected, iid, synth
from tests import _vote_fuzz as vf

pytestmark = pytest.mark.gpu

REL = 1e-12                      # the bound of tests/test_gpu_subset_vote_edges.py: 1e-12 relative, exactly 0.0 where the rational is 0
FIRST = int(os.environ.get("SCV_FUZZ_FIRST", "0"))
VOTE_SEEDS = int(os.environ.get("SCV_FUZZ_VOTE_SEEDS", str(vf.DEFAULT_VOTE_SEEDS)))
EXPECTED_SEEDS = int(os.environ.get("SCV_FUZZ_EXPECTED_SEEDS", "60"))
MIXED_SEEDS = int(os.environ.get("SCV_FUZZ_MIXED_SEEDS", "40"))
SEQUENCE = 12
MIXED_WORK_DIV = 5


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_call(eng, c):
    """The case as a HOST-mode call: the entry's result object."""
    res = c.R if c.shuffled else None
    if c.entry == "resample":
        return eng.resample_prefix(c.pool, c.truth, c.n_valid, c.R, c.vote_seed, tokens=c.tokens, r_begin=c.r_begin, p_offset=c.p_offset, M=c.M)
    if c.entry == "iid":
        return eng.iid_prefix(c.pool, c.truth, c.n_draws, c.R, c.vote_seed, tokens=c.tokens, r_begin=c.r_begin, p_offset=c.p_offset, M=c.M)
    if c.entry == "token_budget":
        return eng.token_budget_prefix(c.pool, c.tokens, c.truth, c.token_budgets, resamples=res, seed=c.vote_seed, r_begin=c.r_begin,
                                       p_offset=c.p_offset, M=c.M, want_cells=c.want_cells)
    if c.entry == "weighted":
        return eng.weighted_prefix(c.pool, c.weights, c.truth, c.n_valid, rule=c.rule, resamples=res, seed=c.vote_seed, r_begin=c.r_begin,
                                   p_offset=c.p_offset, M=c.M, tokens=c.tokens, want_cells=c.want_cells)
    if c.entry == "adaptive":
        return eng.adaptive_prefix(c.pool, c.truth, c.cap, c.need, rule_flags=c.rule_flags, tokens=c.tokens, resamples=res, seed=c.vote_seed,
                                   r_begin=c.r_begin, p_offset=c.p_offset, M=c.M, want_cells=c.want_cells)
    raise KeyError(c.entry)


def previous_buffers(c, want, rng):
    """What the outputs of a DEVICE-mode call hold before it: random non-negative int64 under every summed output, a nonzero pattern under every
    overwritten one.  Returns (device tensors by output name, host copies of the summed ones)."""
    import torch
    bufs, prev = {}, {}
    for name, w in want.items():
        if name in vf.SUMMED:
            prev[name] = rng.integers(0, 2 ** 40, size=w.shape, dtype=np.int64)
            bufs[name] = _dev(prev[name])
        elif name == "cells":
            bufs[name] = torch.full((c.P, c.B, 16), 0xA5, dtype=torch.uint8, device="cuda")
        else:
            bufs[name] = torch.full(w.shape, -0x5A5A5A5A if name == "cell_votes" else -0x5A5A5A5A5A5A, device="cuda",
                                    dtype=torch.int32 if name == "cell_votes" else torch.int64)
    return bufs, prev


def device_call(eng, c, bufs):
    """The case as a DEVICE-mode call into ``bufs``: enqueued only."""
    r_end = c.r_end if c.shuffled else None
    pool, truth, tokens = _dev(c.pool), _dev(c.truth), _dev(c.tokens)
    if c.entry == "resample":
        eng.resample_prefix_device(pool, truth, _dev(c.n_valid), c.r_begin, c.r_end, c.vote_seed, tokens=tokens, p_offset=c.p_offset, **bufs)
    elif c.entry == "iid":
        eng.iid_prefix_device(pool, truth, _dev(c.n_draws), c.r_begin, c.r_end, c.vote_seed, tokens=tokens, p_offset=c.p_offset, **bufs)
    elif c.entry == "token_budget":
        eng.token_budget_prefix_device(pool, tokens, truth, _dev(c.token_budgets), c.r_begin, r_end, c.vote_seed, c.p_offset, **bufs)
    elif c.entry == "weighted":
        eng.weighted_prefix_device(pool, _dev(c.weights), truth, _dev(c.n_valid), c.rule, c.r_begin, r_end, c.vote_seed, c.p_offset, tokens=tokens,
                                   **bufs)
    elif c.entry == "adaptive":
        eng.adaptive_prefix_device(pool, truth, _dev(c.cap), _dev(c.need), _dev(c.rule_flags), tokens, c.r_begin, r_end, c.vote_seed, c.p_offset,
                                   **bufs)
    else:
        raise KeyError(c.entry)


def assert_outputs(c, got, want, prev=None):
    """Every output of the entry against the mirror: got == want, or got == previous + want for the summed outputs of a DEVICE-mode call."""
    # HOST mode: the engine's result holds exactly the outputs the mirror has; DEVICE mode: the buffers were made from the mirror's
    assert set(got) == set(want), (vf.describe(c), sorted(got), sorted(want))
    for name, w in want.items():
        g = got[name]
        if name == "cells":
            for f in vf.CELL_FIELDS:
                assert np.array_equal(g[f], w[f]), (vf.describe(c), name, f)
        else:
            assert np.array_equal(g, w if prev is None or name not in prev else prev[name] + w), (vf.describe(c), name)


def device_outputs(bufs):
    from o1_inference_scaling_laws_amd.engine import cells_from_torch
    return {k: cells_from_torch(v) if k == "cells" else v.cpu().numpy() for k, v in bufs.items()}


def error_word(eng):
    import torch
    word = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    eng.export_error_word(word)
    return int(word.item())


def run_case(eng, c):
    want = vf.mirror_outputs(c)
    try:
        eng.set_option("grid", c.grid)
        if c.device:
            bufs, prev = previous_buffers(c, want, np.random.default_rng((55, c.seed)))
            device_call(eng, c, bufs)
            left = error_word(eng)                                       # in stream order behind the call: what it left in the word
            eng.sync()
            assert left == 0, (vf.describe(c), left)
            assert_outputs(c, device_outputs(bufs), want, prev)
        else:
            assert_outputs(c, vf.outputs_of(c, host_call(eng, c)), want)
            eng.sync()
    except _lib.ScvError as e:                                           # the draws are valid calls: any refusal is a failure, with its shape
        raise AssertionError(f"{vf.describe(c)}: {e}")
    finally:
        eng.set_option("grid", 0)
    assert error_word(eng) == 0, vf.describe(c)


@pytest.mark.parametrize("seed", range(FIRST, FIRST + VOTE_SEEDS))
@pytest.mark.parametrize("entry", vf.LANE_ENTRIES)
def test_random_vote_call_is_bit_exact(hip_engine, entry, seed):
    c = vf.draw(entry, seed)
    if seed % 3 != 2:
        return run_case(hip_engine, c)
    from o1_inference_scaling_laws_amd.engine import Engine
    eng = Engine(timing=bool(seed & 1))                                  # the first call of a fresh context: every allocation on its path
    try:
        run_case(eng, c)
    finally:
        eng.close()


# ---- the exact expected vote ---------------------------------------------------------------------------------------------------------------

def assert_expected(c, score, hit, E, H):
    for p in range(c.P):
        for b in range(c.B):
            for name, got, want in (("score", score[p, b], E[p][b]), ("hit_prob", hit[p, b], H[p][b])):
                if want == 0:
                    assert got == 0.0, (vf.describe(c), name, p, b, got)
                else:
                    assert abs(got - float(want)) <= REL * float(want), (vf.describe(c), name, p, b, got, float(want))


def expected_device_call(eng, c):
    import torch
    score = torch.full((c.P, c.B), float("nan"), dtype=torch.float64, device="cuda")      # overwritten, whatever they held
    hit = torch.full((c.P, c.B), float("nan"), dtype=torch.float64, device="cuda")
    eng.expected_majority_device(_dev(c.pool), _dev(c.truth), _dev(c.n_valid), score=score, hit_prob=hit)
    return score, hit


@pytest.mark.parametrize("seed", range(FIRST, FIRST + EXPECTED_SEEDS))
def test_random_expected_call(hip_engine, seed):
    eng = hip_engine
    c = vf.draw("expected", seed)
    E, H = expected.expected_majority_exact(c.pool, c.truth, c.n_valid)
    try:
        eng.set_option("grid", c.grid)
        if c.device:
            score, hit = expected_device_call(eng, c)
            left = error_word(eng)
            eng.sync()
            assert left == 0
            score, hit = score.cpu().numpy(), hit.cpu().numpy()
        else:
            res = eng.expected_majority(c.pool, c.truth, c.n_valid)
            score, hit = res.score, res.hit_prob
    finally:
        eng.set_option("grid", 0)
    assert_expected(c, score, hit, E, H)
    assert error_word(eng) == 0


# ---- all eight entries on one context --------------------------------------------------------------------------------------------------------

def draw_aggregate(kind, seed):
    """A call of scv_aggregate_i32 / scv_aggregate_prefix_i32 of at most 20 000 votes.  In HOST mode most are served by the one-block path; prefix
    calls over many pools of 1 or 2 votes are not (their cells and cell tokens pass "host_small_kb") and go through the staging pipeline."""
    from types import SimpleNamespace
    rng = np.random.default_rng((9_300_000 + (kind == "aggregate_prefix"), seed))
    N = int(rng.choice([1, 2, 7, 33, 64, 65, 128, 300]))
    B = int(rng.integers(1, 9))
    P = int(rng.integers(1, max(2, 20_000 // (N * (B if kind == "aggregate" else 1)))))
    a, t, tr = synth.fill(P, B if kind == "aggregate" else 1, N, 77_000 + seed, int(rng.integers(0, 6)), want_tokens=True)
    fold = int(rng.choice([0, 0, 3, 40]))
    if fold:
        a, tr = a % fold, (tr % fold).astype(np.int32)
    c = SimpleNamespace(entry=kind, seed=seed, N=N, B=B, P=P, device=bool(rng.random() < 0.5), truth=tr.astype(np.int32))
    c.with_tokens = bool(rng.random() < 0.5)
    c.n_valid = rng.integers(0, N + 2, size=B).astype(np.int32) if kind == "aggregate_prefix" or rng.random() < 0.5 else None
    c.pool = np.ascontiguousarray(a if kind == "aggregate" else a[:, 0, :]).astype(np.int32)
    c.tokens = np.ascontiguousarray(t if kind == "aggregate" else t[:, 0, :]).astype(np.int32) if c.with_tokens else None
    return c


def aggregate_want(c):
    from tests._adapters import OracleEngine
    if c.entry == "aggregate":
        return OracleEngine().aggregate(c.pool, c.truth, tokens=c.tokens, n_valid=c.n_valid)
    return OracleEngine().aggregate_prefix(c.pool, c.truth, c.n_valid, tokens=c.tokens)


def aggregate_host(eng, c):
    if c.entry == "aggregate":
        return eng.aggregate(c.pool, c.truth, tokens=c.tokens, n_valid=c.n_valid)
    return eng.aggregate_prefix(c.pool, c.truth, c.n_valid, tokens=c.tokens)


def aggregate_device(eng, c):
    fn = eng.aggregate_device if c.entry == "aggregate" else eng.aggregate_prefix_device
    if c.entry == "aggregate":
        return fn(_dev(c.pool), _dev(c.truth), tokens=_dev(c.tokens), n_valid=_dev(c.n_valid))
    return fn(_dev(c.pool), _dev(c.truth), _dev(c.n_valid), tokens=_dev(c.tokens))


def aggregate_got(c, out):
    from o1_inference_scaling_laws_amd.engine import AggregateResult, cells_from_torch
    counters, cells, ctok = out
    return AggregateResult.from_counters(counters.cpu().numpy(), c.P, c.B, cells_from_torch(cells), None if ctok is None else ctok.cpu().numpy())


MIXED_ENTRIES = vf.ENTRIES + ("aggregate", "aggregate_prefix")


def reach_first_vote(c):
    """The first budget of the call takes in the whole pool, so the call has work and reads its first vote whatever else was drawn.  (The lane
    bodies flag a vote outside the bins when they stage a row -- resample_encode_row looks at all N votes of it --, not when a walk or a draw
    with replacement happens to index it; the aggregate kernels flag the votes inside a budget.)"""
    if c.entry == "token_budget":
        c.token_budgets = c.token_budgets.copy()
        c.token_budgets[0] = 2 ** 62
    elif c.entry == "aggregate":
        c.n_valid = None
    else:
        field = "n_valid" if c.entry.startswith("aggregate") else vf.BUDGET_FIELD[c.entry]
        setattr(c, field, getattr(c, field).copy())
        getattr(c, field)[0] = c.N


def sequence_of(seed):
    """The 12 calls of sequence ``seed`` (no GPU): (cases, index of the poisoned call or -1, (first call under the forced grid, first call behind
    it, the grid))."""
    rng = np.random.default_rng((9_100_000, seed))
    kinds = [MIXED_ENTRIES[int(k)] for k in rng.integers(0, len(MIXED_ENTRIES), size=SEQUENCE)]
    for e in rng.permutation(len(MIXED_ENTRIES))[: 2 + seed % 3]:         # (every entry is in one sequence in three or more, wherever it falls)
        kinds[int(rng.integers(0, SEQUENCE))] = MIXED_ENTRIES[int(e)]
    poisoned = 5 + seed % 3 if seed % 4 == 1 else -1
    grids = int(rng.integers(2, 6)), int(rng.integers(7, 11)), int(rng.integers(1, 31))
    cases = []
    for i, kind in enumerate(kinds):
        s = 1000 * seed + i
        c = draw_aggregate(kind, s) if kind.startswith("aggregate") else vf.draw(kind, s, work_div=MIXED_WORK_DIV)
        c.grid = 0                                                        # the sequence sets the option itself
        if i == poisoned:
            c.device = True
            c.pool = c.pool.copy()
            c.pool[int(rng.integers(0, c.P)), ..., 0] = int(rng.choice([-1, 1024, 4096]))
            reach_first_vote(c)
        cases.append(c)
    return cases, poisoned, grids


def run_sequence(seed):
    """Runs sequence ``seed`` on a fresh context and checks every call; returns the HOST-mode calls the staging pipeline served."""
    from o1_inference_scaling_laws_amd.engine import Engine
    from tests._adapters import assert_results_equal
    cases, poisoned, (grid_from, grid_to, grid) = sequence_of(seed)
    eng = Engine(timing=bool(seed & 1))
    queued = []
    try:
        for i, c in enumerate(cases):
            if i == grid_from:
                eng.set_option("grid", grid)
            if i == grid_to:
                eng.set_option("grid", 0)
            where = (seed, i, c.entry, "DEVICE" if c.device else "HOST")
            if c.entry.startswith("aggregate"):
                want = aggregate_want(c) if i != poisoned else None
                if c.device:
                    queued.append((i, c, want, aggregate_device(eng, c), None))
                else:
                    assert_results_equal(aggregate_host(eng, c), want, check_tokens=c.with_tokens)
            elif c.entry == "expected":
                E, H = expected.expected_majority_exact(c.pool, c.truth, c.n_valid) if i != poisoned else (None, None)
                if c.device:
                    queued.append((i, c, (E, H), expected_device_call(eng, c), None))
                else:
                    res = eng.expected_majority(c.pool, c.truth, c.n_valid)
                    assert_expected(c, res.score, res.hit_prob, E, H)
            else:
                # the poisoned call's own results are invalid: its shapes come from the mirror all the same
                want = vf.outputs_of(c, vf.mirror(c)) if i == poisoned else vf.mirror_outputs(c)
                if c.device:
                    bufs, prev = previous_buffers(c, want, np.random.default_rng((56, seed, i)))
                    device_call(eng, c, bufs)
                    queued.append((i, c, want, bufs, prev))
                else:
                    try:
                        assert_outputs(c, vf.outputs_of(c, host_call(eng, c)), want)
                    except _lib.ScvError as e:
                        raise AssertionError(f"{where}: {e}")
        if poisoned >= 0:
            with pytest.raises(_lib.DomainError):
                eng.sync()
        eng.sync()                                                        # the one sync of the sequence (the second, clean one after an error)
        assert error_word(eng) == 0
        for i, c, want, out, prev in queued:
            if i == poisoned:
                continue
            if c.entry.startswith("aggregate"):
                assert_results_equal(aggregate_got(c, out), want, check_tokens=c.with_tokens)
            elif c.entry == "expected":
                assert_expected(c, out[0].cpu().numpy(), out[1].cpu().numpy(), *want)
            else:
                assert_outputs(c, device_outputs(out), want, prev)
        return eng.stat("host_pipelined_calls")
    finally:
        eng.set_option("grid", 0)
        eng.close()


@pytest.mark.parametrize("seed", range(FIRST, FIRST + MIXED_SEEDS))
def test_entries_interleaved_on_one_context(seed):
    """12 calls of the eight entries on one fresh context, modes mixed: the staging block resized between HOST calls of different bodies, DEVICE
    launches queued behind them, bodies of one kernel instantiation back to back with different LDS sizes, the grid option changed on the way.
    HOST calls are checked as they return; DEVICE calls are only enqueued and all checked after ONE sync at the end.  One sequence in four
    carries an out-of-domain vote in one DEVICE call in the middle: the sync raises DomainError, every other call is still exactly right, and
    a second sync is clean."""
    run_sequence(seed)


def test_sequence_45_a_pipelined_host_call_behind_a_poisoned_device_call():
    """Sequence 45, outside the default range: call 5 is the DEVICE call with the out-of-domain vote, call 10 a HOST aggregate_prefix over 7136
    pools of 2 votes that the staging pipeline serves.  That path used to end by reading AND CLEARING the context's error word: the HOST call
    raised the DEVICE call's DomainError, and the sync behind it found nothing.  include/scvote.h: a DEVICE-mode domain error is reported at
    scv_sync; a HOST call reports its own votes."""
    cases, poisoned, _ = sequence_of(45)
    c = cases[10]
    assert poisoned == 5 and (c.entry, c.device, c.N, c.B, c.P) == ("aggregate_prefix", False, 2, 7, 7136)
    assert run_sequence(45) >= 1


def test_a_pipelined_host_call_leaves_an_earlier_device_error_to_sync(hip_engine):
    """The same with fixed arguments on the session's context, for both aggregate entries: a DEVICE resample call over a vote of 4096, then a HOST
    call too large for the one-block path -- it returns the oracle's result, the sync behind it raises DomainError, the next one is clean.  And
    the other way round: the pipelined HOST call's own bad vote is raised at that call and leaves nothing for sync."""
    from tests._adapters import OracleEngine, assert_results_equal
    eng = hip_engine
    bad = np.array([[4096, 1, 1, 2]], dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    a, t, tr = synth.fill(7136, 1, 2, 45, 1, want_tokens=True)
    pool, tok = np.ascontiguousarray(a[:, 0, :]), np.ascontiguousarray(t[:, 0, :])
    nv = np.array([2, 0, 1, 3, 2, 1, 2], dtype=np.int32)
    dense = np.ascontiguousarray(np.broadcast_to(pool[:, None, :], (7136, 7, 2)))
    for prefix in (True, False):
        before = eng.stat("host_pipelined_calls")
        eng.resample_prefix_device(_dev(bad), _dev(one), _dev(np.array([4], dtype=np.int32)), 0, 3, 9)
        if prefix:
            got, want = eng.aggregate_prefix(pool, tr, nv, tokens=tok), OracleEngine().aggregate_prefix(pool, tr, nv, tokens=tok)
        else:
            got, want = eng.aggregate(dense, tr, n_valid=nv), OracleEngine().aggregate(dense, tr, n_valid=nv)
        assert eng.stat("host_pipelined_calls") == before + 1
        assert_results_equal(got, want, check_tokens=prefix)
        with pytest.raises(_lib.DomainError):
            eng.sync()
        eng.sync()
        assert error_word(eng) == 0
    pool[7000, 1] = -1
    with pytest.raises(_lib.DomainError):
        eng.aggregate_prefix(pool, tr, nv, tokens=tok)
    assert error_word(eng) == 0
    eng.sync()


# ---- a count of 65535 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 256])
def test_a_count_of_65535_does_not_wrap(hip_engine, N):
    """scvote_iid.hip.h keeps 16-bit counts, two per LDS word: one value drawn 65535 times fills a count to the last bit beside its neighbour."""
    P, R = 3, 5
    nd = np.array([65535, 65534, 1], dtype=np.int32)
    assert nd.max() == iid.MAX_DRAWS
    pool = np.repeat(np.array([[7], [1023], [500]], dtype=np.int32), N, axis=1)
    tr = np.array([7, 1023, 3], dtype=np.int32)                           # two pools are the truth, one is not
    hits = 2
    got = hip_engine.iid_prefix(pool, tr, nd, R, 12345, M=0)
    for b, k in enumerate(nd.tolist()):
        want = np.zeros(1025, dtype=np.int64)
        want[1] = hits * R
        assert np.array_equal(got.tie_class_hits[b], want), (N, k)
        assert got.truth_count_sum[b] == hits * R * k, (N, k)
    if N > 1:                                                             # two values, alternating, the truth the first: both counts near 2^15
        pool = np.tile(np.array([3, 9], dtype=np.int32), (P, N // 2))
        tr = np.full(P, 3, dtype=np.int32)
        want = iid.iid_prefix(pool, tr, nd, 2, 2 + R, 99, M=3)
        got = hip_engine.iid_prefix(pool, tr, nd, R, 99, r_begin=2, M=3)
        assert want.error_bits == 0 and 0 < want.truth_count_sum[0] < P * R * 65535
        assert np.array_equal(got.tie_class_hits, want.tie_class_hits) and np.array_equal(got.truth_count_sum, want.truth_count_sum)
        assert np.array_equal(got.per_resample, want.per_resample)
