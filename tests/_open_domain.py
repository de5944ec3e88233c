"""Shared by tests/test_open_domain_cpu.py and tests/test_gpu_open_domain.py: pools of arbitrary int32 by value class, the order-preserving
relabelling into 0..distinct-1, one call form for the six pool-ordering entries (numpy mirror, HOST mode, DEVICE mode) and the seeded
draws of the fuzz sweep.

The property (SCV_FLAG_OPEN_DOMAIN, include/scvote.h): a flag-on call on (pool, truth) equals the flag-off call of the same entry on
(enc, truth') in every output, bit for bit -- enc[p] = np.unique(pool[p], return_inverse=True)[1] on the signed values, truth'[p] the
truth's code or 1023 when the truth is not in the row (a row of at most 256 votes never holds code 1023)."""
from __future__ import annotations

import numpy as np

from o1_inference_scaling_laws_amd import adaptive, expected, iid, resample, token_budget, weighted

ENTRIES = ("resample", "expected", "token_budget", "weighted", "adaptive", "iid")
HAS_POOL_ORDER = ("token_budget", "weighted", "adaptive")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)        # the edges of 64 lanes x 4 keys
PS = (1, 7, 40)
RS = (None, 3, 64, 70)                                                          # None: pool order (R = 1) where the entry has one, else R = 1
SPECIAL = np.array([I32_MIN, -1, 0, 1023, 1024, I32_MAX], dtype=np.int64)
CLASSES = ("equal", "distinct", "few", "special", "bitpairs", "mixed")


def row_of(rng, N, cls):
    """One row of N int32 votes of a value class (int64 array inside the int32 range)."""
    if cls == "equal":
        return np.full(N, int(rng.choice([I32_MIN, -7, 5, 1024, I32_MAX, int(rng.integers(I32_MIN, I32_MAX))])), dtype=np.int64)
    if cls == "distinct":                                                       # N = 256 reaches code 255
        v = rng.choice(2 ** 20, size=N, replace=False).astype(np.int64) * 4093 + int(rng.integers(I32_MIN, I32_MIN + 2 ** 20))
        return rng.permutation(v)
    if cls == "few":                                                            # duplicates that straddle the 64-lane slices and the 4 keys of one lane
        vals = rng.integers(I32_MIN, I32_MAX, size=int(rng.integers(2, 6)), dtype=np.int64)
        return vals[(np.arange(N) // int(rng.choice([1, 3, 64]))) % len(vals)] if rng.random() < 0.5 else vals[rng.integers(0, len(vals), N)]
    if cls == "special":
        v = SPECIAL[rng.integers(0, len(SPECIAL), N)]
        v[: min(N, len(SPECIAL))] = rng.permutation(SPECIAL)[: min(N, len(SPECIAL))]
        return rng.permutation(v)
    if cls == "bitpairs":                                                       # pairs that differ only in the sign bit (bit 31) or only in bit 0
        base = rng.integers(0, 2 ** 31, size=(N + 3) // 4, dtype=np.int64) & ~np.int64(1)
        four = np.stack([base, base | 1, base - 2 ** 31, (base | 1) - 2 ** 31], axis=1).reshape(-1)
        return rng.permutation(four)[:N]
    v = rng.integers(I32_MIN, I32_MAX, size=N, dtype=np.int64)                 # mixed: random values, a peak, some in-domain ones
    v[rng.random(N) < 0.4] = int(v[0])
    v[rng.random(N) < 0.2] = int(rng.integers(0, 1024))
    return v


def make_pool(rng, P, N, classes=CLASSES):
    """pool int32 [P, N] cycling through the value classes; truth int32 [P] cycling through: present, absent, INT32_MIN (put into the row),
    a negative value of the row when it has one, the row's modal value."""
    pool = np.empty((P, N), dtype=np.int64)
    truth = np.empty(P, dtype=np.int64)
    for p in range(P):
        row = row_of(rng, N, classes[p % len(classes)])
        kind = (p // len(classes) + p) % 5
        if kind == 0:
            t = int(row[rng.integers(0, N)])
        elif kind == 1:                                                         # absent: a value the row does not hold
            t = int(rng.integers(I32_MIN, I32_MAX))
            while (row == t).any():
                t += 1
        elif kind == 2:                                                         # present and equal to INT32_MIN
            t = I32_MIN
            if len(np.unique(row)) == 1:
                row[:] = t
            elif not (row == t).any():
                row[rng.integers(0, N)] = t
        elif kind == 3:
            neg = row[row < 0]
            t = int(neg[0]) if len(neg) else -int(rng.integers(1, 2 ** 31))
        else:
            u, c = np.unique(row, return_counts=True)
            t = int(u[np.argmax(c)])
        pool[p], truth[p] = row, t
    return pool.astype(np.int32), truth.astype(np.int32)


def relabel(pool, truth):
    """(enc int32 [P, N], truth' int32 [P]): the per-row order-preserving relabelling and the truth's code, or 1023 when it is absent."""
    enc = np.empty(pool.shape, dtype=np.int32)
    tcode = np.empty(pool.shape[0], dtype=np.int32)
    for p in range(pool.shape[0]):
        u, inv = np.unique(pool[p].astype(np.int32), return_inverse=True)
        enc[p] = inv.reshape(-1)
        k = int(np.searchsorted(u, truth[p]))
        tcode[p] = k if k < len(u) and u[k] == truth[p] else 1023
    return enc, tcode


def make_case(rng, entry, P, N, R, B=None, classes=CLASSES):
    """A call of ``entry``: dict with pool, truth and the entry's own inputs.  R None: pool order (entries without one: R = 1)."""
    pool, truth = make_pool(rng, P, N, classes)
    B = B or int(rng.integers(1, 5))
    tokens = rng.integers(0, 50, size=(P, N)).astype(np.int32)
    c = {"entry": entry, "pool": pool, "truth": truth, "tokens": tokens, "seed": int(rng.integers(0, 2 ** 31)), "N": N, "P": P,
         "R": R if (R is not None or entry in HAS_POOL_ORDER) else 1, "r_begin": 0, "p_offset": 0}
    ks = np.array([0, 1, N, N + 3], dtype=np.int32)                             # budgets: 0, 1, N and one above N
    if B < 4:
        ks = np.concatenate([rng.permutation(ks)[:B - 1], [int(rng.integers(0, N + 1))]]).astype(np.int32)
    c["nv"] = ks[:B]
    if entry == "token_budget":
        per = int(tokens.sum(axis=1).max())
        c["tb"] = np.array([0, 1, per, per + 5][:B], dtype=np.int64)[rng.permutation(B)]
        c["tb"][0] = int(rng.integers(-1, per + 1)) if B < 4 else c["tb"][0]
    if entry == "weighted":
        c["weights"] = rng.integers(0, 7, size=(P, N)).astype(np.int32)
        c["rule"] = int(rng.integers(0, 2))
    if entry == "adaptive":
        c["cap"] = np.minimum(c["nv"], N + 1).astype(np.int32)
        need = np.stack([adaptive.margin_rule(N, int(m)) for m in rng.integers(1, 4, size=B)]).astype(np.int32)
        need[0] = adaptive.never(N)
        c["need"] = need
        c["flags"] = rng.integers(0, 2, size=B).astype(np.int32)
    if entry == "iid":
        c["nv"] = np.maximum(c["nv"], 0)
        c["nv"][-1] = N + 9                                                     # draws past the size of the pool
    return c


def with_pool(case, pool, truth):
    d = dict(case)
    d["pool"], d["truth"] = pool, truth
    return d


def _pack(**kw):
    return {k: (None if v is None else np.asarray(v)) for k, v in kw.items()}


def run_mirror(c, open_domain):
    """The numpy mirror of the case's entry -> dict of outputs (the names run_engine uses)."""
    e, R = c["entry"], c["R"]
    r0 = c["r_begin"]
    r1 = None if R is None else r0 + R
    M = c["N"] + 1
    od = {"open_domain": open_domain}
    if e == "resample":
        r = resample.resample_prefix(c["pool"], c["truth"], c["nv"], r0, r1, c["seed"], tokens=c["tokens"], p_offset=c["p_offset"], M=M, **od)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, tcs=r.truth_count_sum, per=r.per_resample, err=r.error_bits)
    if e == "iid":
        r = iid.iid_prefix(c["pool"], c["truth"], c["nv"], r0, r1, c["seed"], tokens=c["tokens"], p_offset=c["p_offset"], M=M, **od)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, tcs=r.truth_count_sum, per=r.per_resample, err=r.error_bits)
    if e == "expected":
        s, h = expected.expected_majority_quadrature(c["pool"], c["truth"], c["nv"], **od)
        return _pack(score=s, hit=h, err=int(expected.domain_error(c["pool"], open_domain)))
    if e == "token_budget":
        r = token_budget.token_budget_prefix(c["pool"], c["tokens"], c["truth"], c["tb"], r0, r1, c["seed"], c["p_offset"], M=M, want_cells=R is None, **od)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, votes=r.vote_count_sum, tcs=r.truth_count_sum, per=r.per_resample, cells=r.cells,
                     cell_tokens=r.cell_tokens, err=r.error_bits)
    if e == "weighted":
        r = weighted.weighted_prefix(c["pool"], c["weights"], c["truth"], c["nv"], c["rule"], r0, r1, c["seed"], c["p_offset"], M=M, tokens=c["tokens"],
                                     want_cells=R is None, **od)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, per=r.per_resample, cells=r.cells, cell_tokens=r.cell_tokens, err=r.error_bits)
    r = adaptive.adaptive_prefix(c["pool"], c["truth"], c["cap"], c["need"], c["flags"], c["tokens"], r0, r1, c["seed"], c["p_offset"], M=M,
                                 want_cells=R is None, **od)
    return _pack(tie=r.tie_class_hits, tok=r.token_sum, votes=r.vote_count_sum, tcs=r.truth_count_sum, hist=r.stop_hist, per=r.per_resample,
                 cells=r.cells, cell_tokens=r.cell_tokens, cell_votes=r.cell_votes, err=r.error_bits)


def run_host(eng, c):
    """HOST mode through ``eng`` -> dict of outputs (no ``err``: an error raises)."""
    e, R = c["entry"], c["R"]
    M = c["N"] + 1
    kw = dict(seed=c["seed"], r_begin=c["r_begin"], p_offset=c["p_offset"], M=M)
    if e == "resample":
        r = eng.resample_prefix(c["pool"], c["truth"], c["nv"], R, tokens=c["tokens"], **kw)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, tcs=r.truth_count_sum, per=r.per_resample)
    if e == "iid":
        r = eng.iid_prefix(c["pool"], c["truth"], c["nv"], R, tokens=c["tokens"], **kw)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, tcs=r.truth_count_sum, per=r.per_resample)
    if e == "expected":
        r = eng.expected_majority(c["pool"], c["truth"], c["nv"])
        return _pack(score=r.score, hit=r.hit_prob)
    if e == "token_budget":
        r = eng.token_budget_prefix(c["pool"], c["tokens"], c["truth"], c["tb"], R, want_cells=R is None, **kw)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, votes=r.vote_count_sum, tcs=r.truth_count_sum, per=r.per_resample, cells=r.cells,
                     cell_tokens=r.cell_tokens)
    if e == "weighted":
        r = eng.weighted_prefix(c["pool"], c["weights"], c["truth"], c["nv"], c["rule"], R, tokens=c["tokens"], want_cells=R is None, **kw)
        return _pack(tie=r.tie_class_hits, tok=r.token_sum, per=r.per_resample, cells=r.cells, cell_tokens=r.cell_tokens)
    r = eng.adaptive_prefix(c["pool"], c["truth"], c["cap"], c["need"], c["flags"], c["tokens"], R, want_cells=R is None, **kw)
    return _pack(tie=r.tie_class_hits, tok=r.token_sum, votes=r.vote_count_sum, tcs=r.truth_count_sum, hist=r.stop_hist, per=r.per_resample,
                 cells=r.cells, cell_tokens=r.cell_tokens, cell_votes=r.cell_votes)


def device_inputs(c):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items() if isinstance(v, np.ndarray)}


def launch_device(eng, c, d, bufs=None):
    """One DEVICE-mode call on the tensors ``d`` (device_inputs); ``bufs``: the tuple an earlier call returned, to accumulate into.
    Returns the tuple of output tensors (asynchronous)."""
    e, R = c["entry"], c["R"]
    r0 = c["r_begin"]
    r1 = None if R is None else r0 + R
    M = c["N"] + 1
    b = bufs or ()
    if e in ("resample", "iid"):
        fn = eng.resample_prefix_device if e == "resample" else eng.iid_prefix_device
        names = ("tie_class_hits", "token_sum", "truth_count_sum", "per_resample")
        return fn(d["pool"], d["truth"], d["nv"], r0, r1, c["seed"], tokens=d["tokens"], p_offset=c["p_offset"], M=M, **dict(zip(names, b)))
    if e == "expected":
        return eng.expected_majority_device(d["pool"], d["truth"], d["nv"], **dict(zip(("score", "hit_prob"), b)))
    kw = dict(r_begin=r0, r_end=r1, seed=c["seed"], p_offset=c["p_offset"], M=M, want_cells=R is None)
    if e == "token_budget":
        names = ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "per_resample", "cells", "cell_tokens")
        return eng.token_budget_prefix_device(d["pool"], d["tokens"], d["truth"], d["tb"], **kw, **{n: x for n, x in zip(names, b) if x is not None})
    if e == "weighted":
        names = ("tie_class_hits", "token_sum", "per_resample", "cells", "cell_tokens")
        return eng.weighted_prefix_device(d["pool"], d["weights"], d["truth"], d["nv"], c["rule"], tokens=d["tokens"], **kw,
                                          **{n: x for n, x in zip(names, b) if x is not None})
    names = ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "stop_hist", "per_resample", "cells", "cell_tokens", "cell_votes")
    return eng.adaptive_prefix_device(d["pool"], d["truth"], d["cap"], d["need"], d["flags"], d["tokens"], **kw,
                                      **{n: x for n, x in zip(names, b) if x is not None})


DEVICE_KEYS = {"resample": ("tie", "tok", "tcs", "per"), "iid": ("tie", "tok", "tcs", "per"), "expected": ("score", "hit"),
               "token_budget": ("tie", "tok", "votes", "tcs", "per", "cells", "cell_tokens"),
               "weighted": ("tie", "tok", "per", "cells", "cell_tokens"),
               "adaptive": ("tie", "tok", "votes", "tcs", "hist", "per", "cells", "cell_tokens", "cell_votes")}


def unpack_device(c, outs):
    from o1_inference_scaling_laws_amd.engine import cells_from_torch
    res = {}
    for k, t in zip(DEVICE_KEYS[c["entry"]], outs):
        res[k] = None if t is None else (cells_from_torch(t) if k == "cells" else t.cpu().numpy())
    return res


def run_device(eng, c):
    """DEVICE mode through ``eng`` (fresh zeroed outputs), synchronised -> dict of outputs."""
    outs = launch_device(eng, c, device_inputs(c))
    eng.sync()
    return unpack_device(c, outs)


def assert_equal(got, want, what, skip=(), float_rtol=None):
    """Both hold the same outputs (``err`` apart: only the mirrors report it), each bit for bit (``float_rtol``: float outputs within that
    relative bound instead).  ``skip``: outputs, or "cells.<field>", that are not compared."""
    assert set(got) - {"err"} == set(want) - {"err"}, (what, sorted(got), sorted(want))
    for k, w in want.items():
        if k in skip or k == "err":
            continue
        g = got[k]
        assert (g is None) == (w is None), (what, k)
        if w is None:
            continue
        if k == "cells":
            for f in w.dtype.names:
                if ("cells." + f) not in skip:
                    assert np.array_equal(g[f], w[f]), (what, k, f, g[f].ravel()[:8], w[f].ravel()[:8])
        elif w.dtype.kind == "f" and float_rtol is not None:
            assert np.all(np.abs(g - w) <= float_rtol * np.abs(w)), (what, k, float(np.abs(g - w).max()))
        elif w.dtype.kind == "f":
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, k)
        else:
            assert np.array_equal(g, w), (what, k, np.asarray(g).ravel()[:8], np.asarray(w).ravel()[:8])


def grid_cases(entry, seed=0):
    """One case per N of NS (16).  P = PS[i % 3] and R = RS[i % 4] cycle independently (3 and 4 are coprime, 16 > 12), so every (P, R) pair of
    the grid occurs for the entry: R = 70 at P = 1, 7 and 40, and pool order (entries without one: R = 1) at P = 1, 7 and 40."""
    rng = np.random.default_rng(1000 + seed)
    for i, N in enumerate(NS):
        yield make_case(rng, entry, PS[i % 3], N, RS[i % 4], B=4 if i % 2 == 0 else None)


def fuzz_cases(n=150, seed=20261):
    """The seeded sweep: n draws over entry, shape, R, value class and mode."""
    rng = np.random.default_rng(seed)
    for i in range(n):
        entry = ENTRIES[int(rng.integers(0, len(ENTRIES)))]
        N = int(rng.choice(NS)) if rng.random() < 0.6 else int(rng.integers(1, 257))
        P = int(rng.choice([1, 2, 7, 13]))
        R = [None, 1, 3, 64, 70][int(rng.integers(0, 5))]
        cls = tuple(rng.permutation(CLASSES)[: int(rng.integers(1, len(CLASSES) + 1))])
        yield i, ("host", "device")[int(rng.integers(0, 2))], make_case(rng, entry, P, N, R, classes=cls)
