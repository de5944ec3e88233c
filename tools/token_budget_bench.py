#!/usr/bin/env python3
"""Timing of scv_token_budget_prefix_i32 (the majority vote over the longest prefix of an ordering that fits a token budget) next to
scv_resample_prefix_i32 with tokens at n_valid = N on the same pools: every lane of the token-budget body walks until its largest budget is
spent, so the resample call over whole pools is the work it is held to.

  python tools/token_budget_bench.py [--shapes a,b,c,d] [--reps 5] [--json out.json]

Shapes (budgets 2^11 ... 2^18, 8 of them; synthetic tokens of 100 .. 12 000 per sample, ~780 k per pool of 128): (a) P = 30, N = 128,
R = 10^4 (the reference); (b) P = 10^4, N = 128, R = 10^3; (c) P = 10^4, N = 256, R = 256; (d) the pool order at P = 10^5, N = 128 (next to
the resample call at R = 1).  Kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call, median of --reps.  Run it
under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 10_000), "b": (10_000, 128, 1_000), "c": (10_000, 256, 256), "d": (100_000, 128, None)}
BUDGETS = [2 ** i for i in range(11, 19)]


def timed(eng, fn, reps):
    fn(0)                                                                       # warm-up
    eng.sync()
    eng.drain_kernel_ns()
    out = []
    for rep in range(reps):
        fn(100 + rep)
        eng.sync()
        ns, n = eng.drain_kernel_ns()
        out.append(ns / max(n, 1) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    out = {"budgets": BUDGETS, "shapes": {}}
    with Engine(device=0, timing=True) as eng:
        dev = torch.device("cuda", eng.device)
        for key in args.shapes.split(","):
            P, N, R = SHAPES[key]
            pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tok = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tr = torch.empty((P,), dtype=torch.int32, device=dev)
            eng.synth_fill_device(pool, tok, tr, P=P, B=1, N=N, seed=7, dist=1)
            pool, tok = pool.view(P, N), tok.view(P, N)
            bud = torch.tensor(BUDGETS, dtype=torch.int64, device=dev)
            nv = torch.full((len(BUDGETS),), N, dtype=torch.int32, device=dev)
            r_end = R if R is not None else None
            outs = eng.token_budget_prefix_device(pool, tok, tr, bud, 0, r_end, 1)
            bufs = dict(tie_class_hits=outs[0], token_sum=outs[1], vote_count_sum=outs[2], truth_count_sum=outs[3])
            tb = timed(eng, lambda s: eng.token_budget_prefix_device(pool, tok, tr, bud, 0, r_end, s, **bufs), args.reps)
            rbufs = dict(tie_class_hits=outs[0], token_sum=outs[1], truth_count_sum=outs[3])
            rs = timed(eng, lambda s: eng.resample_prefix_device(pool, tr, nv, 0, R or 1, s, tokens=tok, **rbufs), args.reps)
            # spent / votes of one call, for the record (how far the largest budget walks into the pools)
            one = eng.token_budget_prefix_device(pool, tok, tr, bud, 0, r_end, 1)
            eng.sync()
            cells = P * (R or 1)
            row = {"P": P, "N": N, "R": R, "order": "shuffled" if R else "pool",
                   "mean_pool_tokens": float(tok.to(torch.int64).sum().item()) / P,
                   "avg_votes": [round(float(v) / cells, 2) for v in one[2].cpu().tolist()],
                   "avg_tokens_used": [round(float(v) / cells, 1) for v in one[1].cpu().tolist()],
                   "token_budget_us": round(statistics.median(tb), 1), "token_budget_us_all": [round(x, 1) for x in tb],
                   "resample_n_eq_N_us": round(statistics.median(rs), 1), "resample_us_all": [round(x, 1) for x in rs]}
            row["ratio"] = round(row["token_budget_us"] / row["resample_n_eq_N_us"], 3)
            print(key, json.dumps(row), flush=True)
            out["shapes"][key] = row
            del pool, tok, tr, outs, one
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
