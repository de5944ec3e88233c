"""CPU tests of the adaptive (early-stopping) majority vote (scv_adaptive_prefix_i32): the numpy mirror (o1_inference_scaling_laws_amd/adaptive.py)
against an independent, naive per-ordering loop written from the header (tests/independent_adaptive.py), the kernel's running runner-up
against a sort of the counts, the rule builders' values, the reductions to resample_prefix that must hold bit for bit, the identities of the
stop histogram, the error bits and the source checks.  No GPU needed."""
import os
import re
import sys
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import adaptive, curves, resample, synth
from o1_inference_scaling_laws_amd.adaptive import STOP_DECIDED, beta_rule, margin_rule, never

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import independent_adaptive as ind  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pool_of(P, N, seed, dist=1):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    return a[:, 0, :].copy(), t[:, 0, :].copy(), tr


def rules_for(N, B, seed):
    """ragged caps (negative, 0, inside, N, beyond N), random need tables (values below 0 and above N + 1 too), built rules, both flags."""
    rng = np.random.default_rng(seed)
    cap = rng.choice([-3, 0, 1, max(1, N // 2), N, N + 7] + rng.integers(0, N + 1, size=4).tolist(), size=B).astype(np.int32)
    need = rng.integers(-2, N + 4, size=(B, N + 1)).astype(np.int32)
    built = [never(N), margin_rule(N, 1), margin_rule(N, 2), margin_rule(N, 3), beta_rule(N, 0.9), beta_rule(N, Fraction(19, 20))]
    for b in range(B):
        if rng.random() < 0.6:
            need[b] = built[int(rng.integers(len(built)))]
    flags = rng.integers(0, 2, size=B).astype(np.int32)
    return cap, need, flags


def assert_mirror_is(got, want, cells=False, tokens=True):
    assert np.array_equal(got.tie_class_hits, want["tie"])
    assert np.array_equal(got.vote_count_sum, want["vote_sum"]) and np.array_equal(got.truth_count_sum, want["truth_sum"])
    assert np.array_equal(got.stop_hist, want["stop_hist"]) and np.array_equal(got.per_resample, want["per"])
    if tokens:
        assert np.array_equal(got.token_sum, want["token_sum"])
    else:
        assert got.token_sum is None
    if cells:
        for (p, b), (mx, tc, nm, mm, hit, spent, n) in want["cells"].items():
            c = got.cells[p, b]
            assert (int(c["max_count"]), int(c["truth_count"]), int(c["n_modes"]), int(c["min_mode"]), int(c["hit"])) == (mx, tc, nm, mm, hit), (p, b)
            assert int(got.cell_votes[p, b]) == n and (not tokens or int(got.cell_tokens[p, b]) == spent), (p, b)


@pytest.mark.parametrize("N", [1, 2, 3, 8, 33, 64, 65, 128, 256])
@pytest.mark.parametrize("shuffled", [False, True])
def test_mirror_against_the_independent_loop(N, shuffled):
    for dist in range(6):
        k = N + dist
        B = (1, 5, 32)[k % 3] if N <= 65 else (1, 4)[k % 2]
        P = 4 if N <= 65 else 2
        R = ((1, 3, 7)[k % 3] if N <= 65 else 2) if shuffled else 1
        r0 = (0, 5, 2 ** 31 - 1 - R)[k % 3] if shuffled else 0
        p_off = (0, 9, 1 << 33)[(k + 1) % 3] if shuffled else 0
        pool, tok, tr = pool_of(P, N, 100 + k, dist)
        if dist == 3:
            pool[0, 0], tr[P - 1] = 4096, 5000                           # clamped to bin 1023; a truth outside the bins never hits
        cap, need, flags = rules_for(N, B, k)
        use_tok = k % 4 != 0
        M = N + 1
        got = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok if use_tok else None, r_begin=r0,
                                       r_end=r0 + R if shuffled else None, seed=7 + k, p_offset=p_off, M=M, want_cells=not shuffled)
        want = ind.adaptive(pool, tr, cap, need, flags, tok if use_tok else None, r0, r0 + R if shuffled else None, 7 + k, p_off, M)
        assert_mirror_is(got, want, cells=not shuffled, tokens=use_tok)
        assert got.error_bits == (1 if dist == 3 else 0)


def test_the_running_runner_up_is_the_second_sorted_count():
    """The kernel keeps (maxc, nmodes, sec) per lane and reads c2 = nmodes >= 2 ? maxc : sec (csrc/scvote_adaptive.hip.h).  Run that update
    over random sequences -- few values, many values, long runs of one value -- and compare c1, c2 and nmodes with a sort of the counts after
    every sample."""
    rng = np.random.default_rng(5)
    for trial in range(400):
        n = int(rng.integers(1, 257))
        k = int(rng.choice([1, 2, 3, 5, 17, 256]))
        seq = rng.integers(0, k, size=n)
        if trial % 5 == 0:
            seq = np.sort(seq)
        if trial % 7 == 0:
            seq = np.repeat(seq[: max(1, n // 8)], 8)[:n]
        cnt = Counter()
        maxc = nmodes = sec = 0
        for v in seq.tolist():
            cnt[v] += 1
            c = cnt[v]
            if c > maxc:
                if nmodes > 1:
                    sec = maxc
                maxc, nmodes = c, 1
            elif c == maxc:
                nmodes += 1
            else:
                sec = max(sec, c)
            c2 = maxc if nmodes >= 2 else sec
            counts = sorted(cnt.values(), reverse=True)
            assert maxc == counts[0] and nmodes == counts.count(counts[0])
            assert c2 == (counts[1] if len(counts) > 1 else 0), (trial, seq.tolist())


def test_rule_builder_values():
    assert beta_rule(64, 0.95)[0] == 4                                   # 1 - 2^-4 = 0.9375 < 0.95 <= 1 - 2^-5
    assert beta_rule(64, Fraction(15, 16))[0] == 3 and beta_rule(64, Fraction(15, 16) + Fraction(1, 10 ** 9))[0] == 4
    assert np.array_equal(margin_rule(8, 2), np.arange(9) + 2) and margin_rule(8, 2).dtype == np.int32
    assert np.array_equal(never(5), np.full(6, 6)) and never(5).dtype == np.int32
    for N in (1, 7, 40):
        for conf in (0.5, 0.9, 0.95, 0.99, Fraction(999, 1000)):
            need = beta_rule(N, conf)
            assert need.shape == (N + 1,) and need.dtype == np.int32
            assert (np.diff(need) >= 0).all()                            # monotone in c2
            for c2 in range(N + 1):                                      # the definition, by exhaustive search
                ok = [c1 for c1 in range(c2 + 1, N + 1) if adaptive.beta_confidence(c1, c2) >= Fraction(conf)]
                assert need[c2] == (ok[0] if ok else N + 1), (N, conf, c2)
    assert adaptive.beta_confidence(3, 1) == Fraction(1 + 5 + 10 + 10, 32)
    assert (np.diff(margin_rule(30, 4)) >= 0).all() and (np.diff(beta_rule(256, 0.99)) >= 0).all()
    assert beta_rule(4, 1)[0] == 5                                       # certainty is never reached: N + 1 everywhere
    assert (beta_rule(4, 1) == 5).all()


@pytest.mark.parametrize("dist", range(6))
def test_never_is_the_fixed_vote_and_decided_changes_only_the_cost(dist):
    """`never` with flag 0 is resample_prefix at k = cap, bit for bit; with SCV_STOP_DECIDED the tie classes and per_resample stay (the mode
    cannot change once it is decided) while the votes drawn can only fall."""
    P, N, R, r0, seed, p_off = 6, 48, 9, 3, 11, 4
    pool, tok, tr = pool_of(P, N, 60 + dist, dist)
    cap = np.array([N, 1, 0, 17, -2, N + 5, 30], dtype=np.int32)
    B = len(cap)
    plain = adaptive.adaptive_prefix(pool, tr, cap, never(N), None, tokens=tok, r_begin=r0, r_end=r0 + R, seed=seed, p_offset=p_off, M=N + 1)
    ref = resample.resample_prefix(pool, tr, cap, r0, r0 + R, seed, tokens=tok, p_offset=p_off, M=N + 1)
    assert np.array_equal(plain.tie_class_hits, ref.tie_class_hits) and np.array_equal(plain.per_resample, ref.per_resample)
    assert np.array_equal(plain.token_sum, ref.token_sum) and np.array_equal(plain.truth_count_sum, ref.truth_count_sum)
    nmax = np.clip(cap, 0, N)
    for b in range(B):
        spike = np.zeros(N + 1, dtype=np.int64)
        spike[nmax[b]] = P * R
        assert np.array_equal(plain.stop_hist[b], spike)
    assert np.array_equal(plain.vote_count_sum, nmax.astype(np.int64) * P * R)
    dec = adaptive.adaptive_prefix(pool, tr, cap, never(N), np.full(B, STOP_DECIDED, dtype=np.int32), tokens=tok, r_begin=r0, r_end=r0 + R,
                                   seed=seed, p_offset=p_off, M=N + 1)
    assert np.array_equal(dec.tie_class_hits, plain.tie_class_hits) and np.array_equal(dec.per_resample, plain.per_resample)
    assert (dec.vote_count_sum <= plain.vote_count_sum).all() and (dec.token_sum <= plain.token_sum).all()
    if dist == 2:                                                        # every vote the same: decided after cap // 2 + 1 samples
        assert dec.vote_count_sum[0] < plain.vote_count_sum[0]
        assert np.array_equal(dec.vote_count_sum, np.where(nmax > 0, nmax // 2 + 1, 0).astype(np.int64) * P * R)


@pytest.mark.parametrize("shuffled", [False, True])
def test_stop_histogram_identities(shuffled):
    P, N = 9, 40
    pool, tok, tr = pool_of(P, N, 77, 1)
    cap, need, flags = rules_for(N, 12, 3)
    R = 6 if shuffled else 1
    res = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_end=R if shuffled else None, seed=2, M=N + 1)
    assert (res.stop_hist.sum(axis=1) == P * R).all()
    assert np.array_equal((res.stop_hist * np.arange(N + 1)).sum(axis=1), res.vote_count_sum)
    assert np.allclose(res.stop_distribution(3).sum(), 1.0)
    assert float(res.avg_votes(3)) == res.vote_count_sum[3] / (P * R)
    assert res.exact_accuracy(2) == Fraction(sum(Fraction(int(c), m) for m, c in enumerate(res.tie_class_hits[2]) if m), P * R)
    assert res.resample_accuracy(1).shape == (R,) and np.isclose(res.resample_accuracy(1).mean(), res.accuracy(1))


def test_slices_and_shards_add_up():
    P, N = 7, 33
    pool, tok, tr = pool_of(P, N, 5, 4)
    cap, need, flags = rules_for(N, 6, 8)
    whole = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_begin=2, r_end=12, seed=3, p_offset=10, M=N + 1)
    a = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_begin=2, r_end=5, seed=3, p_offset=10, M=N + 1)
    b = adaptive.adaptive_prefix(pool, tr, cap, need, flags, tokens=tok, r_begin=5, r_end=12, seed=3, p_offset=10, M=N + 1)
    for f in ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "stop_hist"):
        assert np.array_equal(getattr(a, f) + getattr(b, f), getattr(whole, f)), f
    assert np.array_equal(np.concatenate([a.per_resample, b.per_resample]), whole.per_resample)
    s0 = adaptive.adaptive_prefix(pool[:3], tr[:3], cap, need, flags, tokens=tok[:3], r_begin=2, r_end=12, seed=3, p_offset=10, M=N + 1)
    s1 = adaptive.adaptive_prefix(pool[3:], tr[3:], cap, need, flags, tokens=tok[3:], r_begin=2, r_end=12, seed=3, p_offset=13, M=N + 1)
    for f in ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "stop_hist", "per_resample"):
        assert np.array_equal(getattr(s0, f) + getattr(s1, f), getattr(whole, f)), f


def test_need_zero_and_one_stop_at_the_first_sample_and_a_single_row_serves_every_rule():
    pool, tok, tr = pool_of(5, 20, 1, 0)
    for v in (-4, 0, 1):
        res = adaptive.adaptive_prefix(pool, tr, [20, 7], np.full(21, v, dtype=np.int32), tokens=tok)
        assert (res.stop_hist[:, 1] == 5).all() and np.array_equal(res.token_sum, np.full(2, tok[:, 0].sum()))
    res = adaptive.adaptive_prefix(pool, tr, [20, 0], margin_rule(20, 2), want_cells=True)
    assert res.stop_hist[1, 0] == 5 and not res.tie_class_hits[1].any() and (res.cells["min_mode"][:, 1] == -1).all()
    assert not res.cell_votes[:, 1].any() and res.token_sum is None and res.cell_tokens is None


def test_error_bits_and_argument_errors():
    pool, tok, tr = pool_of(3, 8, 2, 3)
    bad = pool.copy()
    bad[1, 2] = -1
    assert adaptive.adaptive_prefix(bad, tr, [8], never(8)).error_bits == 1
    assert adaptive.adaptive_prefix(pool, tr, [8], never(8), [2]).error_bits == adaptive.ERR_RULE_FLAG_BIT
    neg = tok.copy()
    neg[0, 0] = -5                                                       # tokens decide nothing: not an error
    assert adaptive.adaptive_prefix(pool, tr, [8], never(8), tokens=neg).error_bits == 0
    tie8 = np.tile(np.arange(8, dtype=np.int32), (3, 1))
    assert adaptive.adaptive_prefix(tie8, np.array([0, 1, 2]), [8], never(8), r_end=2, M=8).error_bits == 2
    for kw in (dict(cap=[1] * 33), dict(need=np.zeros((1, 8), dtype=np.int32)), dict(rule_flags=[0, 0]), dict(r_begin=1), dict(M=0),
               dict(want_cells=True, r_end=2), dict(tokens=tok[:, :4])):
        args = dict(cap=[8], need=never(8), rule_flags=None)
        args.update(kw)
        cap, need, flags = args.pop("cap"), args.pop("need"), args.pop("rule_flags")
        with pytest.raises(ValueError):
            adaptive.adaptive_prefix(pool, tr, cap, need, flags, **args)
    with pytest.raises(ValueError):
        adaptive.adaptive_prefix(np.zeros((2, 300), dtype=np.int32), [0, 0], [1], never(300))


def test_curve_records_schema():
    class FakeEngine:
        def adaptive_prefix(self, pool, truth, cap, need, flags, tokens=None, resamples=None, seed=0, M=None):
            assert M == 0 and need.shape == (len(cap), pool.shape[1] + 1) and flags.dtype == np.int32
            return adaptive.adaptive_prefix(pool, truth, cap, need, flags, tokens=tokens, r_end=resamples, seed=seed)
    pool, tok, tr = pool_of(6, 16, 4, 1)
    rules = [(16, never(16), 0), (16, margin_rule(16, 2), 0), (16, beta_rule(16, 0.95), STOP_DECIDED)]
    recs = curves.adaptive_vote_records(FakeEngine(), pool, tr, tok, rules, resamples=5, seed=1)
    assert [sorted(r) for r in recs] == [["accuracy", "avg_tokens_used", "avg_votes", "rule"]] * 3
    assert recs[0]["avg_votes"] == 16.0 and recs[1]["avg_votes"] <= 16.0 and recs[1]["avg_tokens_used"] <= recs[0]["avg_tokens_used"]
    assert curves.adaptive_vote_records(FakeEngine(), pool, tr, None, rules)[0]["avg_tokens_used"] == 0.0


def test_header_declares_the_call_and_no_key_was_added():
    hdr = open(os.path.join(REPO, "include", "scvote.h")).read()
    assert re.search(r"\bint scv_adaptive_prefix_i32\(", hdr) and "#define SCV_STOP_DECIDED 0x1" in hdr
    src = open(os.path.join(REPO, "o1_inference_scaling_laws_amd", "csrc", "scvote.hip")).read()
    assert len(re.findall(r"!strcmp\(key,", src)) == 36                  # 16 option keys + 20 stat keys: both lists were full before this call
    assert "adaptive" not in "".join(re.findall(r'!strcmp\(key, "([a-z0-9_]+)"\)', src))
    body = src[src.index("int scv_adaptive_prefix_i32("):]
    assert body[: body.index("\n}\n")].split("{\n", 1)[1].lstrip().startswith("return guarded([&]() -> int {")
    res = open(os.path.join(REPO, "o1_inference_scaling_laws_amd", "csrc", "scvote_resample.hip.h")).read()
    assert res.count("__global__") == 1 and "kResampleModeAdaptive" in res
    assert "__global__" not in open(os.path.join(REPO, "o1_inference_scaling_laws_amd", "csrc", "scvote_adaptive.hip.h")).read()
