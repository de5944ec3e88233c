"""CPU checks of the draw generator behind tests/test_gpu_fuzz_votes.py (tests/_vote_fuzz.py): the default seeds REACH what they are for
(exact conditions on the shapes, modes and LDS layouts, not statistics), the numpy mirrors equal their naive statements on the fuzz's own
small draws, and the draws DISCRIMINATE: deliberately wrong variants of every mirror differ from it on at least a tenth of the draws, so a
kernel wrong in that way would not pass.  No GPU."""
import collections

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import iid, resample, token_budget
from o1_inference_scaling_laws_amd.scoring import exact_accuracy_from_tie_classes
from o1_inference_scaling_laws_amd.synth import G, _MASK32, mix64
from tests import _vote_fuzz as vf
from tests import independent_adaptive, independent_iid, independent_weighted
from tests.test_resample_cpu import scalar_reference
from tests.test_token_budget_cpu import brute

SEEDS = vf.DEFAULT_VOTE_SEEDS     # the default of tests/test_gpu_fuzz_votes.py, from the same constant: the conditions hold for the draws it runs
SMALL = 20_000                   # P * R * N of the draws the naive statements run on
MIN_SMALL = 30
MIN_SHARE = 0.10


@pytest.fixture(scope="module")
def draws():
    return {e: [vf.draw(e, s) for s in range(SEEDS)] for e in vf.LANE_ENTRIES}


def test_a_draw_depends_on_entry_and_seed_alone():
    for e in vf.ENTRIES:
        a, b = vf.draw(e, 5), vf.draw(e, 5)
        assert vars(a).keys() == vars(b).keys()
        for k, v in vars(a).items():
            assert np.array_equal(v, getattr(b, k)) if isinstance(v, np.ndarray) else v == getattr(b, k), (e, k)
    assert vf.draw("resample", 5).vote_seed != vf.draw("iid", 5).vote_seed != vf.draw("iid", 6).vote_seed      # a stream per entry, a state per seed
    assert len({vf.draw(e, s).vote_seed for e in vf.LANE_ENTRIES for s in range(50)}) == 250


# ---- reach ----------------------------------------------------------------------------------------------------------------------------------

def _largest_layout_class(entry):
    """What the body can reach: LDS words grow with N, B and the rows a chunk touches, so the tightest layouts are at N = 256, B = 32, P large."""
    classes = set()
    for shuffled in ((True, False) if entry in vf.HAS_ORDER else (True,)):
        for R in ((1, 2, 3, 63, 64, 65, 600) if shuffled else (1,)):
            fit = vf.lanes_that_fit(entry, 256, 32, R, 700, shuffled)
            assert fit, (entry, R, shuffled)                             # something always fits: no draw is refused for its LDS
            classes.add(str(max(fit)))
    return classes


@pytest.mark.parametrize("entry", vf.LANE_ENTRIES)
def test_the_default_seeds_reach_every_stratum(draws, entry):
    cs = draws[entry]
    need = {
        "N = 1": lambda c: c.N == 1, "N = 256": lambda c: c.N == 256, "N % 4 != 0": lambda c: c.N % 4 != 0,
        "B = 1": lambda c: c.B == 1, "B = 32": lambda c: c.B == 32,
        "R = 1": lambda c: c.R == 1, "R >= 256": lambda c: c.R >= 256,
        "HOST": lambda c: not c.device, "DEVICE": lambda c: c.device,
        "M = 0": lambda c: c.M == 0, "M = N + 1": lambda c: c.M == c.N + 1,
        "all distinct": lambda c: c.pool_kind == "distinct" and all(len(set(r)) == c.N for r in c.pool.tolist()),
        "single value": lambda c: c.pool_kind == "single" and bool((c.pool == c.pool[:, :1]).all()),
        "256 lanes fit": lambda c: vf.fit_class(c) == "256",
        "256 lanes do not fit, 128 do": lambda c: vf.fit_class(c) == "128",
    }
    if entry in vf.HAS_ORDER:
        need["pool order"] = lambda c: not c.shuffled and c.R == 1 and c.want_cells
        need["shuffled order"] = lambda c: c.shuffled and not c.want_cells
    if entry != "token_budget":                                          # a token budget counts tokens: its edges are checked below
        need["a budget of 0"] = lambda c: bool((vf.budgets_of(c) == 0).any())
        need["a budget of N"] = lambda c: bool((vf.budgets_of(c) == c.N).any())
        need["a budget above N"] = lambda c: bool((vf.budgets_of(c) > c.N).any())
    else:
        total = lambda c: c.tokens.astype(np.int64).sum(axis=1)         # noqa: E731
        need["a budget of 0"] = lambda c: bool((c.token_budgets == 0).any())
        need["a budget of the pool's whole cost"] = lambda c: bool(np.isin(c.token_budgets, total(c)).any())
        need["a budget above every pool's cost"] = lambda c: bool((c.token_budgets > total(c).max()).any())
        need["a negative budget"] = lambda c: bool((c.token_budgets < 0).any())
    if entry == "iid":
        need["a budget of 4096"] = lambda c: bool((c.n_draws == 4096).any())
        need["a budget of 1000"] = lambda c: bool((c.n_draws == 1000).any())
    if entry == "weighted":
        need.update({"R < 64 shuffled": lambda c: c.shuffled and c.R < 64, "R = 64 shuffled": lambda c: c.shuffled and c.R == 64,
                     "R > 64 shuffled": lambda c: c.shuffled and c.R > 64, "rule 0": lambda c: c.rule == 0, "rule 1": lambda c: c.rule == 1,
                     "rows at the largest weight": lambda c: bool((c.weights == vf.WEIGHT_MAX).all(axis=1).any()),
                     "rows of weight 0": lambda c: bool((c.weights == 0).all(axis=1).any())})
    if entry == "adaptive":
        need.update({"no rule flags": lambda c: c.rule_flags is None, "STOP_DECIDED": lambda c: c.rule_flags is not None and bool(c.rule_flags.any())})
        for k in ("never", "margin", "beta", "random"):
            need[f"a {k} table"] = lambda c, k=k: k in c.rule_kinds
    if "64" in _largest_layout_class(entry):
        need["only 64 lanes fit"] = lambda c: vf.fit_class(c) == "64"
    missing = [name for name, f in need.items() if not any(f(c) for c in cs)]
    assert not missing, (entry, missing)
    assert "64" in _largest_layout_class("weighted") and "64" in _largest_layout_class("adaptive")


@pytest.mark.parametrize("entry", vf.LANE_ENTRIES)
def test_every_draw_is_a_call_the_entry_accepts(draws, entry):
    for c in draws[entry]:
        assert 1 <= c.N <= 256 and 1 <= c.B <= 32 and c.P >= 1 and c.R >= 1 and c.work <= vf.WORK[entry], vf.describe(c)
        assert c.pool.shape == (c.P, c.N) and c.pool.dtype == np.int32 and c.pool.min() >= 0 and c.pool.max() <= 1023
        assert 0 <= c.r_begin and c.r_end == c.r_begin + c.R < 2 ** 31 and c.p_offset >= 0 and 0 <= c.vote_seed < 2 ** 64
        assert c.shuffled or (c.R == 1 and c.r_begin == 0)
        assert c.tokens is None or (c.tokens.shape == c.pool.shape and c.tokens.min() >= 0)
        assert entry != "token_budget" or c.tokens is not None
        assert entry != "iid" or c.n_draws.max() <= iid.MAX_DRAWS
        assert entry != "weighted" or (c.weights.min() >= 0 and c.weights.max() <= vf.WEIGHT_MAX)
        assert vf.lanes_that_fit(entry, c.N, c.B, c.R, c.P, c.shuffled)


def test_the_expected_draws_cover_the_same_votes_and_budgets():
    cs = [vf.draw("expected", s) for s in range(60)]
    assert {c.device for c in cs} == {False, True}
    assert any(c.N == 1 for c in cs) and any(c.N == 256 for c in cs) and any(c.B == 1 for c in cs) and any(c.B == 32 for c in cs)
    assert any(c.pool_kind == "distinct" for c in cs) and any(c.pool_kind == "single" for c in cs)
    assert all(c.n_valid.shape == (c.B,) and c.pool.shape == (c.P, c.N) for c in cs)


# ---- the mirrors against their naive statements, on the fuzz's own small draws ----------------------------------------------------------------

def _small(cs):
    return [c for c in cs if c.P * c.R * c.N <= SMALL]


def _anchor_resample(c, got):
    tie, tsum, tcsum, per, err = scalar_reference(c.pool.tolist(), c.truth.tolist(), c.n_valid.tolist(), c.r_begin, c.r_end, c.vote_seed,
                                                  tokens=None if c.tokens is None else c.tokens.tolist(), p_offset=c.p_offset, M=c.M or None)
    assert err == 0
    want = dict(tie_class_hits=tie, truth_count_sum=tcsum)
    if c.tokens is not None:
        want["token_sum"] = tsum
    if c.M:
        want["per_resample"] = per
    return want


def _anchor_iid(c, got):
    tie, tsum, tcsum, per, err = independent_iid.iid_prefix(c.pool.tolist(), c.truth.tolist(), c.n_draws.tolist(), c.r_begin, c.r_end, c.vote_seed,
                                                            tokens=None if c.tokens is None else c.tokens.tolist(), p_offset=c.p_offset, M=c.M)
    assert err == 0
    want = dict(tie_class_hits=np.array(tie, dtype=np.int64), truth_count_sum=np.array(tcsum, dtype=np.int64))
    if c.tokens is not None:
        want["token_sum"] = np.array(tsum, dtype=np.int64)
    if c.M:
        want["per_resample"] = np.array(per, dtype=np.int64).reshape(c.R, c.B, c.M)
    return want


def _cells_from(table, P, B):
    from o1_inference_scaling_laws_amd.engine import CELL_DTYPE
    cells = np.zeros((P, B), dtype=CELL_DTYPE)
    for (p, b), v in table.items():
        for f, x in zip(vf.CELL_FIELDS, v[:5]):
            cells[f][p, b] = x
    return cells


def _anchor_token_budget(c, got):
    M = c.M or c.N + 1
    tie, tsum, vsum, tcsum, per, cells = brute(c.pool, c.tokens, c.truth, c.token_budgets.tolist(), c.r_begin, c.r_end if c.shuffled else None,
                                               c.vote_seed, c.p_offset, M)
    want = dict(tie_class_hits=tie, token_sum=tsum, vote_count_sum=vsum, truth_count_sum=tcsum)
    if c.M:
        want["per_resample"] = per
    if not c.shuffled:
        want["cells"] = _cells_from(cells, c.P, c.B)
        want["cell_tokens"] = np.array([[cells[(p, b)][5] for b in range(c.B)] for p in range(c.P)], dtype=np.int64)
    return want


def _anchor_weighted(c, got):
    per = [[[0] * c.M for _ in range(c.B)] for _ in range(c.R)] if c.M else None
    cell_tokens = [[0] * c.B for _ in range(c.P)]
    tie, score, toks, cells = independent_weighted.weighted_prefix(
        c.pool.tolist(), c.weights.tolist(), c.truth.tolist(), c.n_valid.tolist(), c.rule, c.r_begin, c.r_end if c.shuffled else None, c.vote_seed,
        c.p_offset, tokens=None if c.tokens is None else c.tokens.tolist(), per_out=per, cell_tokens_out=cell_tokens)
    table = np.zeros((c.B, 1025), dtype=np.int64)
    for b in range(c.B):
        for m, n in tie[b].items():
            table[b, m] = n
        assert exact_accuracy_from_tie_classes(got["tie_class_hits"][b], c.P * c.R) == score[b] / (c.P * c.R)
    want = dict(tie_class_hits=table)
    if c.tokens is not None:
        want["token_sum"] = np.array(toks, dtype=np.int64)
    if c.M:
        want["per_resample"] = np.array(per, dtype=np.int64).reshape(c.R, c.B, c.M)
    if not c.shuffled:
        want["cells"] = _cells_from({(p, b): cells[p][b] for p in range(c.P) for b in range(c.B)}, c.P, c.B)
        if c.tokens is not None:
            want["cell_tokens"] = np.array(cell_tokens, dtype=np.int64)
    return want


def _anchor_adaptive(c, got):
    flags = np.zeros(c.B, dtype=np.int32) if c.rule_flags is None else c.rule_flags
    w = independent_adaptive.adaptive(c.pool, c.truth, c.cap, c.need, flags, c.tokens, c.r_begin, c.r_end if c.shuffled else None, c.vote_seed,
                                      c.p_offset, c.M or c.N + 1)
    want = dict(tie_class_hits=w["tie"], vote_count_sum=w["vote_sum"], truth_count_sum=w["truth_sum"], stop_hist=w["stop_hist"])
    if c.tokens is not None:
        want["token_sum"] = w["token_sum"]
    if c.M:
        want["per_resample"] = w["per"]
    if not c.shuffled:
        want["cells"] = _cells_from(w["cells"], c.P, c.B)
        want["cell_votes"] = np.array([[w["cells"][(p, b)][6] for b in range(c.B)] for p in range(c.P)], dtype=np.int32)
        if c.tokens is not None:
            want["cell_tokens"] = np.array([[w["cells"][(p, b)][5] for b in range(c.B)] for p in range(c.P)], dtype=np.int64)
    return want


ANCHOR = {"resample": _anchor_resample, "token_budget": _anchor_token_budget, "weighted": _anchor_weighted, "adaptive": _anchor_adaptive,
          "iid": _anchor_iid}


@pytest.mark.parametrize("entry", vf.LANE_ENTRIES)
def test_the_mirror_equals_its_naive_statement_on_the_small_draws(draws, entry):
    small = _small(draws[entry])
    assert len(small) >= MIN_SMALL, (entry, len(small))
    for c in small:
        got = vf.mirror_outputs(c)
        want = ANCHOR[entry](c, got)
        assert set(got) == set(want), (vf.describe(c), sorted(got), sorted(want))
        for k in want:
            if k == "cells":
                for f in vf.CELL_FIELDS:
                    assert np.array_equal(got[k][f], want[k][f]), (vf.describe(c), k, f)
            else:
                assert np.array_equal(got[k], want[k]), (vf.describe(c), k)


# ---- the draws discriminate --------------------------------------------------------------------------------------------------------------

def _late_swap_index(s, r, i, N):
    """resample.swap_index with the stream of every resample started one step late (counter i + 2 where i + 1 is due)."""
    with np.errstate(over="ignore"):
        u = mix64(np.asarray(s, dtype=np.uint64) + G * (np.asarray(r, dtype=np.uint64) * np.uint64(N) + np.uint64(i + 2)))
    return np.uint64(i) + (((u >> np.uint64(32)) & _MASK32) * np.uint64(N - i) >> np.uint64(32))


def _late_draw_index(s, r, i, N):
    with np.errstate(over="ignore"):
        u = mix64(np.asarray(s, dtype=np.uint64) + G * (np.asarray(r, dtype=np.uint64) * np.uint64(iid.R_STRIDE) + np.uint64(i + 2)))
    return ((u >> np.uint64(32)) & _MASK32) * np.uint64(N) >> np.uint64(32)


def _with_late_stream(c, mp):
    mp.setattr(resample, "swap_index", _late_swap_index)
    mp.setattr(token_budget, "swap_index", _late_swap_index)
    mp.setattr(iid, "draw_index", _late_draw_index)
    return vf.outputs_of(c, vf.mirror(c))


def _wrong_tie_class(c, true):
    """a hit that shares the top with others counted one class too low (n_modes - 1 where n_modes >= 2 is due); a unique mode is counted right,
    so the variant shows only on draws whose hits include ties."""
    tie = true["tie_class_hits"]
    wrong = np.zeros_like(tie)
    wrong[:, 1] = tie[:, 1] + tie[:, 2]
    wrong[:, 2:-1] = tie[:, 3:]
    return {**true, "tie_class_hits": wrong}


def _one_sample_short(c, field, N_clamped=True):
    k = getattr(c, field).astype(np.int64)
    k = np.clip(k, 0, c.N) if N_clamped else np.maximum(k, 0)
    return vf.outputs_of(c, vf.mirror(c, **{field: (k - 1).astype(np.int32)}))


WRONG = {
    "resample": {
        "k_b - 1 samples taken": lambda c, true, mp: _one_sample_short(c, "n_valid"),
        "a tied hit counted one class too low": lambda c, true, mp: _wrong_tie_class(c, true),
        "the stream of resample r started one step late": lambda c, true, mp: _with_late_stream(c, mp),
    },
    "token_budget": {
        "budgets read as 32-bit": lambda c, true, mp: vf.outputs_of(c, vf.mirror(c, token_budgets=c.token_budgets.astype(np.int32).astype(np.int64))),
        "a tied hit counted one class too low": lambda c, true, mp: _wrong_tie_class(c, true),
        "budgets too generous by one sample's tokens": lambda c, true, mp: vf.outputs_of(
            c, vf.mirror(c, token_budgets=np.where(c.token_budgets < 2 ** 61, c.token_budgets + c.tokens.max(), c.token_budgets))),
    },
    "weighted": {
        "the maximum taken where the sum is due (and the sum for the maximum)": lambda c, true, mp: vf.outputs_of(c, vf.mirror(c, rule=1 - c.rule)),
        "k_b - 1 samples taken": lambda c, true, mp: _one_sample_short(c, "n_valid"),
        "a tied hit counted one class too low": lambda c, true, mp: _wrong_tie_class(c, true),
    },
    "adaptive": {
        "the cap one sample short": lambda c, true, mp: _one_sample_short(c, "cap"),
        "need read at c2 + 1": lambda c, true, mp: vf.outputs_of(c, vf.mirror(c, need=np.ascontiguousarray(np.roll(c.need, -1, axis=1)))),
        "a tied hit counted one class too low": lambda c, true, mp: _wrong_tie_class(c, true),
    },
    "iid": {
        "budgets clamped to N": lambda c, true, mp: vf.outputs_of(c, vf.mirror(c, n_draws=np.minimum(c.n_draws, c.N))),
        "k_b - 1 samples taken": lambda c, true, mp: _one_sample_short(c, "n_draws", N_clamped=False),
        "the stream of resample r started one step late": lambda c, true, mp: _with_late_stream(c, mp),
    },
}
MUTANT_WORK = {"resample": 400_000, "token_budget": 150_000, "weighted": 150_000, "adaptive": 30_000, "iid": 400_000}
REWRITES = ("a tied hit counted one class too low",)                     # built from the true outputs: no second run of the mirror
REWRITE_WORK = {**MUTANT_WORK, "adaptive": vf.WORK["adaptive"]}          # the adaptive mirror is the slow one: its rewrite runs on every draw


@pytest.mark.parametrize("entry", vf.LANE_ENTRIES)
def test_wrong_variants_of_the_mirror_differ_on_a_tenth_of_the_draws(draws, entry):
    """The variants that run the mirror again do so on the draws below MUTANT_WORK only (the whole range would take minutes), the rewrites of
    the true outputs on those below REWRITE_WORK; every share is counted over ALL default draws, so what is asserted is a lower bound of the
    true share."""
    cs = [c for c in draws[entry] if c.work <= REWRITE_WORK[entry]]
    differ = collections.Counter()
    for c in cs:
        true = vf.mirror_outputs(c)
        for name, wrong in WRONG[entry].items():
            if name not in REWRITES and c.work > MUTANT_WORK[entry]:
                continue
            with pytest.MonkeyPatch.context() as mp:
                differ[name] += not vf.same_outputs(wrong(c, true, mp), true)
    shares = {name: differ[name] / SEEDS for name in WRONG[entry]}
    print(entry, {k: round(v, 3) for k, v in shares.items()})
    assert all(s >= MIN_SHARE for s in shares.values()), (entry, f"{len(cs)} of {SEEDS} draws run", shares)
