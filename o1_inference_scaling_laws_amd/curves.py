"""Accuracy-vs-token-budget curves from resampled majority votes (Engine.resample_prefix, include/scvote.h
scv_resample_prefix_i32).

The reference's majority-vote tail (o1.py:266-277: T >= 2^11 votes over the first N = T // 2^11 samples of the 2^11-token pool)
is one ordering of the cache.  ``expected_majority_records`` averages each point over ``resamples`` random orderings of the same
pool and returns it in the reference's log schema, so plot_helpers can draw the smoothed tail next to the single-ordering one.
``wide_majority_records`` is the same average for pools of up to 4096 samples (Engine.resample_wide).
``exact_majority_records`` gives the limit of that average -- the mean over all k-subsets -- with no seed and no resample count.
``token_budget_records`` ends each vote where a budget of TOKENS runs out instead of after a number of samples;
``adaptive_vote_records`` where a stopping rule on the vote's own state says it is settled.  ``iid_majority_records`` draws WITH
replacement, so its curve goes on past the size of the pool, and ends in the k -> infinity limit."""
from __future__ import annotations

import numpy as np

from .o1_dropin import majority_vote_budgets

KEY_LIMIT = 2 ** 11          # o1.py:274: actual_token_limit = min(2 ** 11, token_limit)


def resampled_budgets(token_limits=None, shade_regions: bool = False):
    """[(token_limit, N)] of the budgets that vote over prefixes of the 2^11-token pool (o1_dropin.majority_vote_budgets)."""
    if token_limits is None:
        return [(t, n) for t, key, n in majority_vote_budgets(shade_regions) if key == KEY_LIMIT]
    out = []
    for t in token_limits:
        t = int(t)
        if t < KEY_LIMIT:
            raise ValueError(f"token_limit {t} < 2^11 votes over one sample of its own pool, not over a prefix of the 2^11-token pool")
        out.append((t, t // KEY_LIMIT))
    return out


def expected_majority_records(engine, pool, truth, tokens, token_limits, resamples: int, seed: int):
    """pool / tokens int32 [P, Npool] (the 2^11-token samples of each problem, in cache order), truth int32 [P].  For every
    token limit T >= 2^11: the expected accuracy of the majority vote over N = T // 2^11 samples drawn without replacement
    (average over ``resamples`` orderings) and the expected tokens used, as records
    {'token_limit', 'accuracy', 'avg_tokens_used'} (o1.py:278-283).  ``tokens`` may be None (avg_tokens_used is then 0.0)."""
    budgets = resampled_budgets(token_limits)
    pool = np.asarray(pool, dtype=np.int32)
    ns = np.array([n for _t, n in budgets], dtype=np.int32)
    if len(ns) and ns.max() > pool.shape[1]:
        raise ValueError(f"token limit {budgets[int(ns.argmax())][0]} needs {int(ns.max())} samples per problem; the pool has {pool.shape[1]}")
    res = engine.resample_prefix(pool, truth, ns, resamples, seed, tokens=tokens, M=0)
    return [{"token_limit": t, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b))}
            for b, (t, _n) in enumerate(budgets)]


def wide_majority_records(engine, pool, truth, tokens, token_limits, resamples: int, seed: int):
    """As expected_majority_records for pools of up to 4096 samples per problem (Engine.resample_wide, scv_resample_wide_i32): the same
    records {'token_limit', 'accuracy', 'avg_tokens_used'} (o1.py:278-283) for T >= 2^11, N = T // 2^11 <= Npool.  The orderings are drawn by
    sort keys, not by the shuffle of expected_majority_records: the two curves agree in expectation, not draw by draw.  ``tokens`` may be None
    (avg_tokens_used is then 0.0).  With an ``Engine(open_domain=True)`` the pool may hold any int32 (scv_resample_wide_i32 under
    SCV_FLAG_OPEN_DOMAIN)."""
    budgets = resampled_budgets(token_limits)
    pool = np.asarray(pool, dtype=np.int32)
    ns = np.array([n for _t, n in budgets], dtype=np.int32)
    if len(ns) and ns.max() > pool.shape[1]:
        raise ValueError(f"token limit {budgets[int(ns.argmax())][0]} needs {int(ns.max())} samples per problem; the pool has {pool.shape[1]}")
    res = engine.resample_wide(pool, truth, ns, resamples, seed, tokens=tokens, M=0)
    return [{"token_limit": t, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b))}
            for b, (t, _n) in enumerate(budgets)]


def exact_majority_records(engine, pool, truth, tokens, token_limits):
    """As expected_majority_records, but each point is the exact mean over all N-subsets of the pool (Engine.expected_majority,
    scv_expected_majority_i32): records {'token_limit', 'accuracy', 'avg_tokens_used'} (o1.py:278-283) for T >= 2^11, N = T // 2^11.
    ``tokens`` may be None (avg_tokens_used is then 0.0)."""
    budgets = resampled_budgets(token_limits)
    pool = np.asarray(pool, dtype=np.int32)
    ns = np.array([n for _t, n in budgets], dtype=np.int32)
    if len(ns) and ns.max() > pool.shape[1]:
        raise ValueError(f"token limit {budgets[int(ns.argmax())][0]} needs {int(ns.max())} samples per problem; the pool has {pool.shape[1]}")
    res = engine.expected_majority(pool, truth, ns, tokens=tokens, hit_prob=False)
    return [{"token_limit": t, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b))}
            for b, (t, _n) in enumerate(budgets)]


def token_budget_records(engine, pool, truth, tokens, token_limits, resamples: int | None = None, seed: int = 0):
    """pool / tokens int32 [P, Npool] (each problem's samples in cache order), truth int32 [P].  For every token limit T: the accuracy of
    the majority vote over the longest prefix whose tokens fit T (Engine.token_budget_prefix, scv_token_budget_prefix_i32) -- in the
    cache order (``resamples=None``, one draw) or averaged over ``resamples`` random orderings -- and the tokens it actually spent, as
    records {'token_limit', 'accuracy', 'avg_tokens_used'} (o1.py:278-283).  Here token_limit is a real per-problem cap:
    avg_tokens_used <= token_limit, so plot_helpers can draw the curve beside the maj@N tail on the same axis."""
    limits = [int(t) for t in token_limits]
    res = engine.token_budget_prefix(np.asarray(pool, dtype=np.int32), np.asarray(tokens, dtype=np.int32), truth,
                                     np.array(limits, dtype=np.int64), resamples=resamples, seed=seed, M=0)
    return [{"token_limit": t, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b))}
            for b, t in enumerate(limits)]


def wide_token_budget_records(engine, pool, truth, tokens, token_limits, resamples: int | None = None, seed: int = 0):
    """``token_budget_records`` for caches of up to WIDE_MAX_N = 4096 samples per problem (Engine.token_budget_wide,
    scv_token_budget_wide_i32): pool / tokens int32 [P, Npool], truth int32 [P].  For every token limit T -- any number of them; the engine
    takes 32 per call -- the accuracy of the majority vote over the longest prefix whose tokens fit T, in the cache order (``resamples=None``)
    or averaged over ``resamples`` sorted-key orderings, the tokens it spent and the samples it voted over, as records {'token_limit',
    'accuracy', 'avg_tokens_used', 'avg_votes'}: the token axis of o1.py:266-283 up to 2^22 and beyond.  At Npool <= 256 the shuffled
    orderings differ from those of ``token_budget_records`` (only the expectation is shared); the cache order gives the same records."""
    limits = [int(t) for t in token_limits]
    pool = np.asarray(pool, dtype=np.int32)
    tokens = np.asarray(tokens, dtype=np.int32)
    recs = []
    for i in range(0, len(limits), 32):
        part = limits[i:i + 32]
        res = engine.token_budget_wide(pool, tokens, truth, np.array(part, dtype=np.int64), resamples=resamples, seed=seed, M=0)
        recs += [{"token_limit": t, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b)), "avg_votes": float(res.avg_votes(b))}
                 for b, t in enumerate(part)]
    return recs


def shortest_vote_records(engine, pool, truth, tokens, pairs, resamples: int | None = None, seed: int = 0):
    """pool / tokens int32 [P, Npool] (each problem's samples in cache order), truth int32 [P], ``pairs`` a list of (k, m).  For every pair:
    the accuracy of short-m@k -- k samples in parallel, the vote over the m that finish first (Engine.shortest_prefix,
    scv_shortest_prefix_i32) -- in the cache order (``resamples=None``, one draw) or averaged over ``resamples`` random orderings, against the
    compute it spends and against its latency, as records {'k', 'm', 'accuracy', 'avg_tokens_used' (spent: the kept chains, and every other
    chain up to the moment the m-th finishes), 'avg_voted_tokens', 'avg_latency' (the m-th shortest chain)}.  At most 32 pairs per call of
    the engine; longer lists are split."""
    pairs = [(int(k), int(m)) for k, m in pairs]
    pool = np.asarray(pool, dtype=np.int32)
    tokens = np.asarray(tokens, dtype=np.int32)
    recs = []
    for i in range(0, len(pairs), 32):
        part = pairs[i:i + 32]
        res = engine.shortest_prefix(pool, tokens, truth, [k for k, _ in part], [m for _, m in part], resamples=resamples, seed=seed, M=0)
        recs += [{"k": k, "m": m, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_spent_tokens(b)),
                  "avg_voted_tokens": float(res.avg_voted_tokens(b)), "avg_latency": float(res.avg_latency(b))} for b, (k, m) in enumerate(part)]
    return recs


def weighted_majority_records(engine, pool, weights, truth, tokens, token_limits, rule, resamples: int | None = None, seed: int = 0):
    """pool / weights / tokens int32 [P, Npool] (the 2^11-token samples of each problem in cache order, each with an integer weight in
    0 .. WEIGHT_MAX: weighted.quantize_weights), truth int32 [P].  For every token limit T >= 2^11 (the budgets of resampled_budgets,
    N = T // 2^11 samples): the accuracy of the weighted majority vote (``rule`` RULE_WEIGHT_SUM) or of best-of-N (RULE_BEST_OF) over the
    first N samples -- of the cache order (``resamples=None``, one draw) or averaged over ``resamples`` random orderings -- and the tokens
    used (Engine.weighted_prefix, scv_weighted_prefix_i32), as records {'token_limit', 'accuracy', 'avg_tokens_used'} (o1.py:278-283):
    the curve drops into plot_helpers next to the plain vote's.  ``tokens`` may be None (avg_tokens_used is then 0.0)."""
    budgets = resampled_budgets(token_limits)
    pool = np.asarray(pool, dtype=np.int32)
    ns = np.array([n for _t, n in budgets], dtype=np.int32)
    if len(ns) and ns.max() > pool.shape[1]:
        raise ValueError(f"token limit {budgets[int(ns.argmax())][0]} needs {int(ns.max())} samples per problem; the pool has {pool.shape[1]}")
    res = engine.weighted_prefix(pool, weights, truth, ns, rule=rule, resamples=resamples, seed=seed, M=0, tokens=tokens)
    return [{"token_limit": t, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b))}
            for b, (t, _n) in enumerate(budgets)]


def adaptive_vote_records(engine, pool, truth, tokens, rules, resamples: int | None = None, seed: int = 0):
    """pool / tokens int32 [P, Npool] (each problem's samples in cache order; tokens may be None), truth int32 [P].  ``rules``: a list of
    (cap, need, flags) -- the most samples the rule may draw, its stopping table int32 [Npool + 1] (adaptive.never / margin_rule /
    beta_rule) and 0 or STOP_DECIDED.  For every rule: the accuracy of the vote that samples until the rule stops it
    (Engine.adaptive_prefix, scv_adaptive_prefix_i32) -- in the cache order (``resamples=None``, one draw) or averaged over ``resamples``
    random orderings -- and what it actually spent, as records {'rule', 'accuracy', 'avg_votes', 'avg_tokens_used'}: accuracy against
    samples or tokens spent is the curve of a stopping policy (avg_tokens_used is 0.0 without tokens)."""
    pool = np.asarray(pool, dtype=np.int32)
    cap = np.array([int(c) for c, _n, _f in rules], dtype=np.int32)
    need = np.stack([np.asarray(n, dtype=np.int32) for _c, n, _f in rules])
    flags = np.array([int(f) for _c, _n, f in rules], dtype=np.int32)
    res = engine.adaptive_prefix(pool, truth, cap, need, flags, tokens=tokens, resamples=resamples, seed=seed, M=0)
    return [{"rule": b, "accuracy": res.accuracy(b), "avg_votes": float(res.avg_votes(b)),
             "avg_tokens_used": float(res.avg_tokens_used(b)) if tokens is not None else 0.0} for b in range(len(rules))]


def iid_majority_records(engine, pool, truth, tokens, draws, resamples: int, seed: int, token_limits=None):
    """pool / tokens int32 [P, Npool] (each problem's samples; tokens may be None), truth int32 [P].  For every k in ``draws`` (any k up to
    IID_MAX_DRAWS = 65535, also above Npool): the accuracy of the majority vote over k answers drawn WITH replacement from the pool -- the
    plug-in estimate of maj@k, averaged over ``resamples`` draw sequences (Engine.iid_prefix, scv_iid_prefix_i32) -- and the tokens of the
    draws, as records {'samples': k, 'accuracy', 'avg_tokens_used'} (avg_tokens_used is 0.0 without tokens).  The last record is
    {'samples': inf, 'accuracy'}: the k -> infinity limit, which is the vote over the whole pool (Engine.aggregate_prefix at k = Npool).
    With ``token_limits`` (each >= 2^11, the reference's grid: resampled_budgets) instead of ``draws`` (None), k = T // 2^11 whatever the
    size of the pool, and every record but the last also carries 'token_limit'."""
    pool = np.asarray(pool, dtype=np.int32)
    if token_limits is not None:
        if draws is not None:
            raise ValueError("give draws or token_limits, not both")
        budgets = resampled_budgets(token_limits)
        draws = [n for _t, n in budgets]
    draws = [int(k) for k in draws]
    recs = []
    if draws:
        res = engine.iid_prefix(pool, truth, np.array(draws, dtype=np.int32), resamples, seed, tokens=tokens, M=0)
        for b, k in enumerate(draws):
            rec = {"samples": k, "accuracy": res.accuracy(b), "avg_tokens_used": float(res.avg_tokens_used(b)) if tokens is not None else 0.0}
            if token_limits is not None:
                rec["token_limit"] = budgets[b][0]
            recs.append(rec)
    whole = engine.aggregate_prefix(pool, truth, np.array([pool.shape[1]], dtype=np.int32), want_cells=False)
    recs.append({"samples": float("inf"), "accuracy": whole.accuracy(0)})
    return recs
