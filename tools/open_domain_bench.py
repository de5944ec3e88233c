#!/usr/bin/env python3
"""Timing of the open answer domain (SCV_FLAG_OPEN_DOMAIN): the same call on the same synthetic D1 pools through a flag-on and a flag-off
context, and -- ``--siblings`` -- the flag-off lane bodies alone, for A/B runs of two builds of the library (SCV_LIB_PATH).

  python tools/open_domain_bench.py [--shapes a,b,c,d,e] [--reps 5] [--json out.json]
  python tools/open_domain_bench.py --siblings [--reps 5]

Shapes (peaked pools, D1, with tokens; budgets the powers of two 1, 2, 4, ..., N -- the reference's grid; B <= 32 rules out all of 1..128): (a) scv_resample_prefix_i32 at P = 30, N = 128, R = 10^4; (b) the same entry at
P = 10^4, N = 128, R = 10^3; (c) at P = 10^4, N = 256, R = 256; (d) pool order at P = 10^5, N = 128 through scv_token_budget_prefix_i32;
(e) scv_expected_majority_i32 at P = 10^4, N = 128.  The pools lie inside 0..1023, so both contexts compute the same thing: the flag-on one
pays the open encoder, which ranks by counting whatever the values are.  ``--siblings``: the plain shuffle, the weighted vote, the
token-budget body and the adaptive body at P = 30, N = 128, R = 10^4 on a flag-off context.  Kernel time from SCV_FLAG_TIMING
(scv_drain_kernel_ns) after one warm-up call, median of --reps, microseconds.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": ("resample", 30, 128, 10_000), "b": ("resample", 10_000, 128, 1_000), "c": ("resample", 10_000, 256, 256),
          "d": ("token_budget_pool", 100_000, 128, 1), "e": ("expected", 10_000, 128, 1)}


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


def pools(eng, torch, P, N):
    dev = torch.device("cuda", eng.device)
    pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
    tok = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
    tr = torch.empty((P,), dtype=torch.int32, device=dev)
    eng.synth_fill_device(pool, tok, tr, P=P, B=1, N=N, seed=7, dist=1)
    return pool.view(P, N), tok.view(P, N), tr


def call_of(eng, torch, kind, pool, tok, tr, R):
    """A closure seed -> one DEVICE-mode call of ``kind`` that accumulates into buffers of its own."""
    P, N = pool.shape
    dev = pool.device
    nv = torch.tensor([1 << i for i in range(N.bit_length()) if (1 << i) <= N], dtype=torch.int32, device=dev)
    B = int(nv.shape[0])
    if kind == "resample":
        o = eng.resample_prefix_device(pool, tr, nv, 0, R, 1, tokens=tok)
        return lambda s: eng.resample_prefix_device(pool, tr, nv, 0, R, s, tokens=tok, tie_class_hits=o[0], token_sum=o[1], truth_count_sum=o[2])
    if kind == "expected":
        o = eng.expected_majority_device(pool, tr, nv)
        return lambda s: eng.expected_majority_device(pool, tr, nv, score=o[0], hit_prob=o[1])
    if kind in ("token_budget", "token_budget_pool"):
        tb = (nv.to(torch.int64) * int(tok.to(torch.int64).sum().item() // (P * N))).contiguous()
        r_end = None if kind.endswith("pool") else R
        o = eng.token_budget_prefix_device(pool, tok, tr, tb, 0, r_end, 1)
        return lambda s: eng.token_budget_prefix_device(pool, tok, tr, tb, 0, r_end, s, tie_class_hits=o[0], token_sum=o[1], vote_count_sum=o[2],
                                                        truth_count_sum=o[3])
    if kind == "weighted":
        w = (tok % 7 + 1).contiguous()
        o = eng.weighted_prefix_device(pool, w, tr, nv, 0, 0, R, 1, tokens=tok)
        return lambda s: eng.weighted_prefix_device(pool, w, tr, nv, 0, 0, R, s, tokens=tok, tie_class_hits=o[0], token_sum=o[1])
    from o1_inference_scaling_laws_amd import adaptive
    need = torch.from_numpy(__import__("numpy").stack([adaptive.margin_rule(N, 1 + b % 4) for b in range(B)]).astype("int32")).to(dev)
    o = eng.adaptive_prefix_device(pool, tr, nv, need, tokens=tok, r_begin=0, r_end=R, seed=1)
    return lambda s: eng.adaptive_prefix_device(pool, tr, nv, need, tokens=tok, r_begin=0, r_end=R, seed=s, tie_class_hits=o[0], token_sum=o[1],
                                                vote_count_sum=o[2], truth_count_sum=o[3], stop_hist=o[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d,e")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--siblings", action="store_true")
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    out = {"lib": os.environ.get("SCV_LIB_PATH") or "in-tree", "rows": {}}
    if args.siblings:
        with Engine(device=0, timing=True) as eng:
            pool, tok, tr = pools(eng, torch, 30, 128)
            for kind in ("resample", "weighted", "token_budget", "adaptive"):
                us = timed(eng, call_of(eng, torch, kind, pool, tok, tr, 10_000), args.reps)
                row = {"P": 30, "N": 128, "R": 10_000, "us": round(statistics.median(us), 1), "us_all": [round(x, 1) for x in us]}
                print("sibling", kind, json.dumps(row), flush=True)
                out["rows"][kind] = row
    else:
        with Engine(device=0, timing=True) as off, Engine(device=0, timing=True, open_domain=True) as on:
            for key in args.shapes.split(","):
                kind, P, N, R = SHAPES[key]
                pool, tok, tr = pools(off, torch, P, N)
                row = {"entry": kind, "P": P, "N": N, "R": R}
                for name, eng in (("off", off), ("on", on), ("off2", off), ("on2", on)):   # alternating: drift shows as off against off2
                    us = timed(eng, call_of(eng, torch, kind, pool, tok, tr, R), args.reps)
                    row[name + "_us"] = round(statistics.median(us), 1)
                    row[name + "_us_all"] = [round(x, 1) for x in us]
                row["on_over_off"] = round((row["on_us"] + row["on2_us"]) / (row["off_us"] + row["off2_us"]), 3)
                print(key, json.dumps(row), flush=True)
                out["rows"][key] = row
                del pool, tok, tr
                torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
