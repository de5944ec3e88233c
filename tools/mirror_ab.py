"""A/B of the numpy vote mirrors between two trees (no GPU, numpy and the package alone).

    python tools/mirror_ab.py --tree PATH --out DUMP        run every mirror of the package under PATH over a fixed grid; writes DUMP.npz (every
                                                            output array) and DUMP.json (error_bits, absent outputs, refusals: type and text)
    python tools/mirror_ab.py --compare A B                 assert the dumps A and B equal entry by entry: names, dtypes, shapes, values, texts

The grid is a function of this file alone (one seeded generator per case), so two trees see the same calls.  It covers, per mirror: P in
{0, 1, 3, 17} x N in {1, 2, 7, 64, 256} (wide pair: P in {0, 1, 3} x N in {1, 257, 1024, 4096}) x both orders x M in {None, 1, 3, N + 1}, with B in
{1, 3, 32} (duplicate, zero, negative and beyond-range budgets), (r_begin, R) in {0, 5} x {0, 1, 4}, p_offset in {0, 9}, tokens absent / present,
cells on / off and both answer domains rotated over them; a lane-block boundary inside a problem's rows (P = 70, R = 60, N = 5); rows that raise
every error bit; every refusal; and a few draws of tests/_vote_fuzz.py for the five lane entries."""
from __future__ import annotations

import argparse
import dataclasses
import itertools
import json
import sys

import numpy as np

WEIGHT_MAX = 2 ** 24 - 1
ENTRIES = ("resample", "iid", "wide", "wide_budget", "token_budget", "weighted", "adaptive", "shortest")
HAS_ORDER = ("wide_budget", "token_budget", "weighted", "adaptive", "shortest")
WIDE = ("wide", "wide_budget")


def budgets(rng, B: int, N: int, rot: int, top: int | None = None) -> np.ndarray:
    """int32 [B]: beyond the range, zero, negative, a duplicate pair, the ends; random ones after them; rotated so that B = 1 sees each in turn."""
    top = N if top is None else top
    edges = [top + 1, 0, -3, max(top // 2, 1), max(top // 2, 1), top, 1, top - 1]
    edges = edges[rot % len(edges):] + edges[:rot % len(edges)]
    more = rng.integers(0, top + 2, size=max(B - len(edges), 0)).tolist()
    return np.array((edges + more)[:B], dtype=np.int32)


def token_budgets(rng, B: int, tok: np.ndarray, rot: int) -> np.ndarray:
    total = tok.astype(np.int64).clip(0).sum(axis=1) if tok.size else np.zeros(1, dtype=np.int64)
    hi = int(total.max()) if total.size else 0
    edges = [hi + 3, 0, -5, hi // 2, hi // 2, hi, 2 ** 62, int(total[0]) if total.size else 0]
    edges = edges[rot % len(edges):] + edges[:rot % len(edges)]
    more = rng.integers(0, hi + 2, size=max(B - len(edges), 0)).tolist()
    return np.array((edges + more)[:B], dtype=np.int64)


def data(rng, P: int, N: int, open_domain: bool, rot: int):
    """pool, tokens, weights [P, N] and truth [P]: few bins on two cases in three (ties), a truth of the row / absent / outside the bins."""
    fold = (2, 5, 1024)[rot % 3]
    pool = rng.integers(0, fold, size=(P, N))
    if open_domain:
        pool = pool * 100_003 - 2 ** 30                                   # any int32, negative ones among them
    truth = pool[np.arange(P), rng.integers(0, N, size=P)].copy() if P else np.zeros(0, dtype=np.int64)
    if P and rot % 4 == 1:
        truth[::2] = 1023 if rot % 8 == 1 else -3
    tok = rng.integers(0, 50, size=(P, N))
    tok[rng.random((P, N)) < 0.2] = 0
    wts = rng.integers(0, 4, size=(P, N)) if rot % 2 else rng.integers(0, WEIGHT_MAX + 1, size=(P, N))
    return pool.astype(np.int32), tok.astype(np.int32), wts.astype(np.int32), truth.astype(np.int32)


def need_rows(mods, rng, B: int, N: int, rot: int) -> np.ndarray:
    a = mods["adaptive"]
    rows = [a.never(N), a.margin_rule(N, 1 + rot % 3), rng.integers(-2, N + 4, size=N + 1).astype(np.int32)]
    return np.ascontiguousarray(np.stack([rows[(b + rot) % 3] for b in range(B)]), dtype=np.int32)


def call(mods, entry: str, c: dict):
    """One call of ``entry``'s mirror from the case dictionary (every mirror takes its own subset)."""
    m = mods[entry]
    r_end = c["r_begin"] + c["R"] if c["shuffled"] else None
    kw = dict(p_offset=c["p_offset"], M=c["M"], open_domain=c["open_domain"])
    if entry in ("resample", "iid", "wide"):
        f = {"resample": "resample_prefix", "iid": "iid_prefix", "wide": "resample_wide"}[entry]
        return getattr(m, f)(c["pool"], c["truth"], c["budgets"], c["r_begin"], c["r_begin"] + c["R"], c["seed"], tokens=c["tokens"], **kw)
    kw.update(r_begin=c["r_begin"], r_end=r_end, seed=c["seed"], want_cells=c["want_cells"])
    if entry == "wide_budget":
        return m.token_budget_wide(c["pool"], c["tokens"], c["truth"], c["budgets"], **kw)
    if entry == "token_budget":
        return m.token_budget_prefix(c["pool"], c["tokens"], c["truth"], c["budgets"], **kw)
    if entry == "weighted":
        return m.weighted_prefix(c["pool"], c["weights"], c["truth"], c["budgets"], c["rule"], tokens=c["tokens"], **kw)
    if entry == "adaptive":
        return m.adaptive_prefix(c["pool"], c["truth"], c["budgets"], c["need"], c["rule_flags"], c["tokens"], **kw)
    return m.shortest_prefix(c["pool"], c["tokens"], c["truth"], c["budgets"], c["m_keep"], **kw)


def case(mods, entry: str, n: int, P: int, N: int, shuffled: bool, M, B: int, r_begin: int, R: int, p_offset: int, with_tokens: bool,
         want_cells: bool, open_domain: bool) -> dict:
    rng = np.random.default_rng((91_000 + ENTRIES.index(entry), n))
    pool, tok, wts, truth = data(rng, P, N, open_domain, n)
    needs_tokens = entry in ("wide_budget", "token_budget", "shortest")
    c = dict(pool=pool, truth=truth, tokens=tok if with_tokens or needs_tokens else None, weights=wts, rule=n % 2, shuffled=shuffled,
             r_begin=r_begin if shuffled else 0, R=R if shuffled else 1, p_offset=p_offset, M=(0 if entry == "iid" else None) if M is None else M,
             seed=int(rng.integers(0, 2 ** 63)), want_cells=want_cells and not shuffled and entry in HAS_ORDER, open_domain=open_domain)
    if entry in ("wide_budget", "token_budget"):
        c["budgets"] = token_budgets(rng, B, tok, n)
    elif entry == "iid":
        c["budgets"] = budgets(rng, B, N, n, top=2 * N)
    else:
        c["budgets"] = budgets(rng, B, N, n)
    c["m_keep"] = budgets(rng, B, N, n + 3)
    c["need"] = need_rows(mods, rng, B, N, n) if entry == "adaptive" else None
    c["rule_flags"] = None if n % 3 == 0 else rng.integers(0, 2, size=B).astype(np.int32)
    return c


def grid(mods, entry: str):
    """(name, case) for the regular grid of ``entry``: the product of P, N, order and M, the other axes rotated over it with coprime periods."""
    Ps, Ns = ((0, 1, 3), (1, 257, 1024, 4096)) if entry in WIDE else ((0, 1, 3, 17), (1, 2, 7, 64, 256))
    orders = (False, True) if entry in HAS_ORDER else (True,)
    n = 0
    for P, N, shuffled, Mi in itertools.product(Ps, Ns, orders, range(4)):
        for rep in range(2):
            M = (None, 1, 3, N + 1)[Mi]
            B = (1, 3, 32)[n % 3]
            r_begin, R = (0, 5)[n % 2], (0, 1, 4)[(n // 2) % 3]
            if entry in WIDE and N == 4096 and B == 32:
                B = 3                                                     # (32 budgets over 4096-sample orderings: a minute per case, nothing new)
            c = case(mods, entry, n, P, N, shuffled, M, B, r_begin, R, (0, 9)[(n // 5) % 2], bool((n // 7) % 2), bool((n // 3) % 2), bool((n // 11) % 2))
            yield f"grid{n:04d} P={P} N={N} B={B} shuffled={int(c['shuffled'])} r=[{c['r_begin']},+{c['R']}) M={c['M']} p_offset={c['p_offset']} " \
                  f"tok={int(c['tokens'] is not None)} cells={int(c['want_cells'])} open={int(c['open_domain'])}", c
            n += 1


def specials(mods, entry: str):
    """The block boundary, the rows that raise the error bits, the fuzz draws are added by the caller."""
    base = dict(n=5000, P=3, N=7, shuffled=True, M=8, B=3, r_begin=5, R=4, p_offset=9, with_tokens=True, want_cells=False, open_domain=False)
    if entry in ("token_budget", "weighted", "adaptive", "shortest"):
        yield "block boundary P=70 R=60 N=5", case(mods, entry, 5001, 70, 5, True, 6, 3, 5, 60, 9, True, False, False)
    c = case(mods, entry, **base)
    c["pool"] = c["pool"].copy()
    c["pool"][0, 0], c["pool"][2, 3] = -1, 5000
    yield "a vote outside 0..1023", c
    yield "a vote outside 0..1023, open domain", {**c, "open_domain": True}
    for order in ((True, False) if entry in HAS_ORDER else (True,)):
        c = case(mods, entry, **{**base, "n": 5002, "M": 1, "shuffled": order, "want_cells": True})
        yield f"a hit with n_modes >= M (M=1) shuffled={int(order)}", c
    if entry in ("token_budget", "shortest", "wide_budget"):
        c = case(mods, entry, **{**base, "n": 5003})
        c["tokens"] = c["tokens"].copy()
        c["tokens"][1, 2] = -4
        yield "a negative token", c
        yield "a negative token, pool order with cells", {**c, "shuffled": False, "r_begin": 0, "R": 1, "want_cells": True}
    if entry == "weighted":
        c = case(mods, entry, **{**base, "n": 5004})
        c["weights"] = c["weights"].copy()
        c["weights"][0, 1], c["weights"][1, 0] = -1, WEIGHT_MAX + 1
        yield "a weight outside 0..WEIGHT_MAX", c
    if entry == "adaptive":
        c = case(mods, entry, **{**base, "n": 5005})
        c["rule_flags"] = np.array([0, 2, 1], dtype=np.int32)
        yield "an unknown rule flag", c
    if entry == "iid":
        c = case(mods, entry, **{**base, "n": 5006})
        c["budgets"] = np.array([3, mods["iid"].MAX_DRAWS + 1, 0], dtype=np.int32)
        yield "n_draws above MAX_DRAWS", c
        yield "n_draws above MAX_DRAWS, no lanes", {**c, "R": 0}
    if entry in WIDE:
        c = case(mods, entry, **{**base, "n": 5007, "P": 2, "N": 1100, "M": 1101, "open_domain": True, "B": 1})
        c["pool"] = (np.arange(2 * 1100, dtype=np.int64).reshape(2, 1100) * 7 - 5000).astype(np.int32)      # 1100 distinct values a row: all tied
        c["truth"] = c["pool"][:, 3].copy()
        c["budgets"] = np.array([2 ** 62], dtype=np.int64) if entry == "wide_budget" else np.array([1100], dtype=np.int32)
        yield "open domain, more than 1024 distinct values all tied", c
        yield "open domain, more than 1024 distinct values all tied, pool order", {**c, "shuffled": False, "r_begin": 0, "R": 1, "want_cells": entry == "wide_budget"}


def refusals(mods, entry: str):
    """Every refusal of the mirror, each one broken thing on an otherwise valid call."""
    base = dict(n=6000, P=3, N=7, shuffled=True, M=8, B=3, r_begin=0, R=2, p_offset=0, with_tokens=True, want_cells=False, open_domain=False)
    ok = case(mods, entry, **base)
    max_n = 4096 if entry in WIDE else 256
    yield "a 1-D pool", {**ok, "pool": ok["pool"][0]}
    yield "M below its minimum", {**ok, "M": -1 if entry == "iid" else 0}
    yield "a truth of the wrong shape", {**ok, "truth": ok["truth"][:2]}
    yield "tokens of the wrong shape", {**ok, "tokens": ok["tokens"][:, :5]}
    yield "N above the maximum", case(mods, entry, **{**base, "P": 1, "N": max_n + 1})
    yield "B = 33", case(mods, entry, **{**base, "B": 33})
    yield "B = 0", {**ok, "budgets": ok["budgets"][:0], "m_keep": ok["m_keep"][:0], "need": None if ok["need"] is None else ok["need"][:0],
                    "rule_flags": None}
    yield "r_end below r_begin", {**ok, "r_begin": 4, "R": -2}
    yield "a negative p_offset", {**ok, "p_offset": -1}
    if entry in HAS_ORDER:
        pool_order = {**ok, "shuffled": False}
        yield "r_begin != 0 in pool order", {**pool_order, "r_begin": 5, "call_r_begin": 5}
        yield "cells with a shuffled order", {**ok, "want_cells": True}
        yield "r_begin != 0 in pool order and every later fault", {**pool_order, "call_r_begin": 5, "M": 0, "truth": ok["truth"][:2], "rule": 7}
        yield "cells with a shuffled order and M = 0", {**ok, "want_cells": True, "M": 0}
    if entry == "weighted":
        yield "a bad rule", {**ok, "rule": 2}
        yield "a bad rule and a bad shape", {**ok, "rule": -1, "truth": ok["truth"][:2]}
        yield "weights of the wrong shape", {**ok, "weights": ok["weights"][:, :5]}
        yield "no weights", {**ok, "weights": None}
    if entry == "shortest":
        yield "n_valid and m_keep of different lengths", {**ok, "m_keep": ok["m_keep"][:2]}
    if entry == "adaptive":
        yield "a need of the wrong shape", {**ok, "need": ok["need"][:, :5]}
        yield "rule flags of the wrong length", {**ok, "rule_flags": np.zeros(5, dtype=np.int32)}


def call_case(mods, entry: str, c: dict):
    if "call_r_begin" in c:                                              # pool order drops r_begin in ``case``: put the faulty one back
        c = {**c, "r_begin": c["call_r_begin"]}
    return call(mods, entry, c)


def fuzz_cases(tree: str, seeds: int):
    """The first ``seeds`` draws of tests/_vote_fuzz.py (the tree's own copy) for the five lane entries, at a twentieth of their work."""
    from tests import _vote_fuzz as vf
    for entry in vf.LANE_ENTRIES:
        for seed in range(seeds):
            c = vf.draw(entry, seed, work_div=20)
            yield entry, f"fuzz seed={seed} {vf.describe(c)}", vf.mirror(c)


def record(arrays: dict, meta: dict, key: str, res) -> None:
    for f in dataclasses.fields(res):
        v = getattr(res, f.name)
        if isinstance(v, np.ndarray):
            arrays[f"{key} :: {f.name}"] = v
        else:
            meta[f"{key} :: {f.name}"] = None if v is None else int(v)


def run(tree: str, out: str, fuzz_seeds: int) -> None:
    sys.path.insert(0, tree)
    import importlib
    mods = {e: importlib.import_module(f"o1_inference_scaling_laws_amd.{e}") for e in ENTRIES}
    assert all(m.__file__.startswith(tree.rstrip("/") + "/") for m in mods.values()), "the package was not imported from --tree"
    arrays, meta = {}, {}
    for entry in ENTRIES:
        for name, c in itertools.chain(grid(mods, entry), specials(mods, entry)):
            record(arrays, meta, f"{entry} :: {name}", call_case(mods, entry, c))
        for name, c in refusals(mods, entry):
            try:
                res = call_case(mods, entry, c)
                record(arrays, meta, f"{entry} :: accepted: {name}", res)         # (a mirror without that check: the outputs are compared)
            except Exception as e:                                               # noqa: BLE001 -- whatever it raises is the thing compared
                meta[f"{entry} :: refused: {name}"] = f"{type(e).__name__}: {e}"
        print(entry, "done", flush=True)
    for entry, name, res in fuzz_cases(tree, fuzz_seeds):
        record(arrays, meta, f"{entry} :: {name}", res)
    np.savez_compressed(out + ".npz", **arrays)
    with open(out + ".json", "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True)
    print(f"{len(arrays)} arrays and {len(meta)} scalars / refusals -> {out}.npz, {out}.json")


def compare(a: str, b: str) -> int:
    A, B = np.load(a + ".npz"), np.load(b + ".npz")
    with open(a + ".json") as f:
        ma = json.load(f)
    with open(b + ".json") as f:
        mb = json.load(f)
    diffs = []
    for k in sorted(set(A.files) | set(B.files)):
        if k not in A.files or k not in B.files:
            diffs.append(f"{k}: only in {'A' if k in A.files else 'B'}")
        elif A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes():
            diffs.append(f"{k}: {A[k].dtype}{A[k].shape} against {B[k].dtype}{B[k].shape}" + ("" if A[k].shape != B[k].shape else ", values differ"))
    for k in sorted(set(ma) | set(mb)):
        if ma.get(k, "<absent>") != mb.get(k, "<absent>"):
            diffs.append(f"{k}: {ma.get(k, '<absent>')!r} against {mb.get(k, '<absent>')!r}")
    print(f"{'entry':<14}{'calls':>8}{'refusals':>10}{'arrays':>9}{'error_bits != 0':>17}")
    for entry in ENTRIES:
        keys = [k for k in ma if k.startswith(entry + " :: ")]
        calls = {k.rsplit(" :: ", 1)[0] for k in keys if " :: refused: " not in k}
        print(f"{entry:<14}{len(calls):>8}{sum(' :: refused: ' in k for k in keys):>10}{sum(k.startswith(entry + ' :: ') for k in A.files):>9}"
              f"{sum(k.endswith(' :: error_bits') and ma[k] != 0 for k in keys):>17}")
    bits = sorted({ma[k] for k in ma if k.endswith(" :: error_bits")})
    print("error_bits values seen:", bits)
    print("refusal texts seen:", len({v for k, v in ma.items() if " :: refused: " in k}))
    for d in diffs[:50]:
        print("DIFF", d)
    print(f"{len(diffs)} differences")
    return 1 if diffs else 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", help="the tree whose package is run (put first on sys.path)")
    ap.add_argument("--out", help="stem of the dump: OUT.npz and OUT.json")
    ap.add_argument("--fuzz-seeds", type=int, default=8)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="stems of two dumps")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not (args.tree and args.out):
        ap.error("--tree PATH --out DUMP, or --compare A B")
    import os
    run(os.path.abspath(args.tree), args.out, args.fuzz_seeds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
