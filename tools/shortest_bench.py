#!/usr/bin/env python3
"""Timing of scv_shortest_prefix_i32 (short-m@k: the majority vote over the m shortest of the first k samples of an ordering) next to
scv_resample_prefix_i32 with tokens at n_valid = N on the same pools: both walk whole pools, the short-m@k body sets a rank bit per step and
walks m set bits per budget where the resample body counts a vote per step.

  python tools/shortest_bench.py [--shapes a,b,c,d] [--reps 5] [--json out.json]
  python tools/shortest_bench.py --siblings [--pool-size 128] [--label parent] [--reps 5]

Shapes (D1 pools with the synthetic tokens of 100 .. 12 000 per sample): (a) P = 30, N = 128, R = 10^4 (the reference); (b) P = 10^4,
N = 128, R = 10^3; (c) P = 10^4, N = 256, R = 256; (d) the pool order at P = 10^5, N = 128 (next to the resample call at R = 1).  Pairs
(k, m) = (k, 1), (k, ceil(k / 4)), (k, k) for k = 1, 2, 4, ..., N: all of them in one call, and each of the three families in a call of its
own.  The yardstick has as many budgets, all of them N.  Kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call,
median of --reps.  ``--siblings``: flag-off calls of the five other lane bodies alone (the plain shuffle, the weighted vote, the token
budgets, the adaptive vote, the draws with replacement) at P = 30, N = --pool-size, R = 10^4, and the token budgets in pool order at
P = 10^5, for A/B runs of two builds of the library (SCV_LIB_PATH; --label names the build in the output).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 10_000), "b": (10_000, 128, 1_000), "c": (10_000, 256, 256), "d": (100_000, 128, None)}


def families(N):
    ks = [1 << i for i in range(N.bit_length()) if (1 << i) <= N]
    return {"m=1": [(k, 1) for k in ks], "m=k/4": [(k, (k + 3) // 4) for k in ks], "m=k": [(k, k) for k in ks]}


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


def siblings(torch, Engine, reps, N, label):
    sys.path.insert(0, os.path.join(R_, "tools"))
    from open_domain_bench import call_of, pools
    P, R = 30, 10_000
    with Engine(device=0, timing=True) as eng:
        pool, tok, tr = pools(eng, torch, P, N)
        nv = torch.tensor([1 << i for i in range(N.bit_length())], dtype=torch.int32, device=pool.device)
        o = eng.iid_prefix_device(pool, tr, nv, 0, R, 1, tokens=tok)
        calls = {kind: call_of(eng, torch, kind, pool, tok, tr, R) for kind in ("resample", "weighted", "token_budget", "adaptive")}
        calls["iid"] = lambda s: eng.iid_prefix_device(pool, tr, nv, 0, R, s, tokens=tok, tie_class_hits=o[0], token_sum=o[1], truth_count_sum=o[2])
        for kind, fn in calls.items():
            us = timed(eng, fn, reps)
            print("sibling", kind, json.dumps({"P": P, "N": N, "R": R, "lib": label, "us": round(statistics.median(us), 1),
                                               "us_all": [round(x, 1) for x in us]}), flush=True)
        big = pools(eng, torch, 100_000, N)                                     # pool order: one lane per problem
        us = timed(eng, call_of(eng, torch, "token_budget_pool", *big, 1), reps)
        print("sibling", "token_budget_pool", json.dumps({"P": 100_000, "N": N, "R": None, "lib": label, "us": round(statistics.median(us), 1),
                                                         "us_all": [round(x, 1) for x in us]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--siblings", action="store_true")
    ap.add_argument("--pool-size", type=int, default=128)
    ap.add_argument("--label", default="in-tree")
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    if args.siblings:
        siblings(torch, Engine, args.reps, args.pool_size, args.label)
        return
    out = {"shapes": {}}
    with Engine(device=0, timing=True) as eng:
        dev = torch.device("cuda", eng.device)
        for key in args.shapes.split(","):
            P, N, R = SHAPES[key]
            pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tok = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tr = torch.empty((P,), dtype=torch.int32, device=dev)
            eng.synth_fill_device(pool, tok, tr, P=P, B=1, N=N, seed=7, dist=1)
            pool, tok = pool.view(P, N), tok.view(P, N)
            fam = families(N)
            fam["all"] = [p for f in ("m=1", "m=k/4", "m=k") for p in fam[f]]
            r_end = R if R is not None else None
            cells = P * (R or 1)
            row = {"P": P, "N": N, "R": R, "order": "shuffled" if R else "pool", "pairs": fam["all"]}
            nv_full = torch.full((len(fam["all"]),), N, dtype=torch.int32, device=dev)
            first = eng.resample_prefix_device(pool, tr, nv_full, 0, R or 1, 1, tokens=tok)
            rbufs = dict(tie_class_hits=first[0], token_sum=first[1], truth_count_sum=first[2])
            rs = timed(eng, lambda s: eng.resample_prefix_device(pool, tr, nv_full, 0, R or 1, s, tokens=tok, **rbufs), args.reps)
            row["resample_n_eq_N_us"] = round(statistics.median(rs), 1)
            row["resample_us_all"] = [round(x, 1) for x in rs]
            for name, pairs in fam.items():
                nv = torch.tensor([k for k, _ in pairs], dtype=torch.int32, device=dev)
                mk = torch.tensor([m for _, m in pairs], dtype=torch.int32, device=dev)
                outs = eng.shortest_prefix_device(pool, tok, tr, nv, mk, 0, r_end, 1)
                bufs = dict(tie_class_hits=outs[0], voted_token_sum=outs[1], spent_token_sum=outs[2], latency_sum=outs[3], truth_count_sum=outs[4])
                ts = timed(eng, lambda s: eng.shortest_prefix_device(pool, tok, tr, nv, mk, 0, r_end, s, **bufs), args.reps)
                row[f"shortest_{name}_us"] = round(statistics.median(ts), 1)
                row[f"shortest_{name}_us_all"] = [round(x, 1) for x in ts]
                row[f"ratio_{name}"] = round(row[f"shortest_{name}_us"] / row["resample_n_eq_N_us"], 3)
                if name == "all":                                               # one call's curve, for the record
                    one = eng.shortest_prefix_device(pool, tok, tr, nv, mk, 0, r_end, 1)
                    eng.sync()
                    row["avg_spent_tokens"] = [round(float(v) / cells, 1) for v in one[2].cpu().tolist()]
                    row["avg_latency"] = [round(float(v) / cells, 1) for v in one[3].cpu().tolist()]
            print(key, json.dumps(row), flush=True)
            out["shapes"][key] = row
            del pool, tok, tr
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
