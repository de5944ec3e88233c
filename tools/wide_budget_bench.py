#!/usr/bin/env python3
"""Timing of scv_token_budget_wide_i32 (the vote over the longest prefix of an ordering of a pool of up to 4096 samples that fits a token
budget) next to scv_resample_wide_i32 with tokens -- the walk it extends -- on the same pools in the same run, alternating rep by rep.

  python tools/wide_budget_bench.py [--shapes a,b,c,pool] [--reps 5]

Shapes (D1 pools with the synthetic tokens, token budgets 2^11 ... 2^22: a few samples to the whole pool): (a) P = 30, N = 1024, R = 10^3;
(b) P = 30, N = 4096, R = 10^3; (c) P = 10^3, N = 1024, R = 10^2; (pool) P = 10^4, N = 1024 in pool order (no wide counterpart: one draw).
Per shape, kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call, median of --reps:
  budget_us        the token-budget call, 12 budgets
  wide_us          scv_resample_wide_i32 with tokens, sample budgets 1, 2, 4 ... N (the ``tok`` rows of tools/wide_bench.py)
  wide_sort_us     the same with every sample budget 0: the sort of every item and nothing else
  budget_empty_us  the token-budget call with every budget -1: the sort, the scan and the searches, no walk
  budget_whole_us  ... with every budget 2^62: the sort, the scan, the searches and ONE walk over the whole pool
so scan + searches ~ budget_empty_us - wide_sort_us, and the walks are what is left.  ``open``: the same calls on a SCV_FLAG_OPEN_DOMAIN
context (same pools), and its ratio to the flag-off time.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)
sys.path.insert(0, os.path.join(R_, "tools"))

SHAPES = {"a": (30, 1024, 1_000), "b": (30, 4096, 1_000), "c": (1_000, 1024, 100), "pool": (10_000, 1024, None)}
LDS_BYTES = 160 * 1024


def launch_shape(N, B, open_domain):
    """(lanes, LDS bytes, workgroups per CU that the LDS ALONE allows) of a launch (the geometry: tools/wide_bench.py, which
    tests/test_wide_budget_cpu.py holds to the header).  The kernel's registers allow 28 waves per CU, 7 workgroups of 256 lanes, which is
    the bound where the LDS would allow more."""
    from wide_bench import wide_budget_lds_words, wide_lanes
    lds = 4 * wide_budget_lds_words(N, B, open_domain)
    return wide_lanes(N), lds, LDS_BYTES // lds


def drain_us(eng):
    eng.sync()
    ns, n = eng.drain_kernel_ns()
    return ns / max(n, 1) / 1e3


def alternating(eng, fns, reps):
    """{name: [us per rep]}: one warm-up call each, then the calls in turn, rep by rep."""
    for fn in fns.values():
        fn(0)
    drain_us(eng)
    out = {k: [] for k in fns}
    for rep in range(reps):
        for k, fn in fns.items():
            fn(100 + rep)
            out[k].append(drain_us(eng))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,pool")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    from resample_bench import pool_for
    with Engine(device=0, timing=True) as eng, Engine(device=0, timing=True, open_domain=True) as oeng:
        for key in args.shapes.split(","):
            P, N, R = SHAPES[key]
            pool, tok, tr = pool_for(eng, P, N, 7)
            dev = pool.device
            limits = [1 << k for k in range(11, 23)]
            B = len(limits)
            bud = torch.tensor(limits, dtype=torch.int64, device=dev)
            empty = torch.full((B,), -1, dtype=torch.int64, device=dev)
            whole = torch.full((B,), 1 << 62, dtype=torch.int64, device=dev)
            nvl = [1 << k for k in range(N.bit_length()) if (1 << k) <= N]
            nv = torch.tensor(nvl, dtype=torch.int32, device=dev)
            nv0 = torch.zeros_like(nv)
            r_end = R                                                            # None: pool order
            row = {"P": P, "N": N, "R": R, "B": B, "mean_tokens": round(float(tok.float().mean()), 1)}
            for label, e in (("plain", eng), ("open", oeng)):
                lanes, lds, per_cu = launch_shape(N, B, label == "open")
                o = e.token_budget_wide_device(pool, tok, tr, bud, 0, r_end, 1)
                bb = dict(tie_class_hits=o[0], token_sum=o[1], vote_count_sum=o[2], truth_count_sum=o[3])
                fns = {"budget_us": lambda s, e=e, bb=bb: e.token_budget_wide_device(pool, tok, tr, bud, 0, r_end, s, **bb),
                       "budget_empty_us": lambda s, e=e, bb=bb: e.token_budget_wide_device(pool, tok, tr, empty, 0, r_end, s, **bb),
                       "budget_whole_us": lambda s, e=e, bb=bb: e.token_budget_wide_device(pool, tok, tr, whole, 0, r_end, s, **bb)}
                if R is not None:
                    w = e.resample_wide_device(pool, tr, nv, 0, R, 1, tokens=tok)
                    wb = dict(tie_class_hits=w[0], token_sum=w[1], truth_count_sum=w[2])
                    fns["wide_us"] = lambda s, e=e, wb=wb: e.resample_wide_device(pool, tr, nv, 0, R, s, tokens=tok, **wb)
                    fns["wide_sort_us"] = lambda s, e=e, wb=wb: e.resample_wide_device(pool, tr, nv0, 0, R, s, tokens=tok, **wb)
                us = alternating(e, fns, args.reps)
                med = {k: round(statistics.median(v), 1) for k, v in us.items()}
                rec = dict(med, lanes=lanes, lds_bytes=lds, workgroups_per_cu_by_lds=per_cu, us_all={k: [round(x, 1) for x in v] for k, v in us.items()})
                f = e.token_budget_wide_device(pool, tok, tr, bud, 0, r_end, 1)
                e.sync()
                rec["avg_votes"] = [round(float(x) / (P * (R or 1)), 1) for x in f[2].cpu().tolist()]
                if R is not None:
                    rec["budget_over_wide"] = round(med["budget_us"] / med["wide_us"], 3)
                    rec["scan_and_searches_us"] = round(med["budget_empty_us"] - med["wide_sort_us"], 1)
                rec["walks_us"] = round(med["budget_us"] - med["budget_empty_us"], 1)
                row[label] = rec
            row["open_over_plain"] = round(row["open"]["budget_us"] / row["plain"]["budget_us"], 3)
            print(key, json.dumps(row), flush=True)
            del pool, tok, tr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
