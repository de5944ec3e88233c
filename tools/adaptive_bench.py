#!/usr/bin/env python3
"""Timing of scv_adaptive_prefix_i32 (the majority vote that samples until a stopping rule says it is settled) next to
scv_resample_prefix_i32 with tokens at n_valid = N on the same pools: the fixed-N walk a stopping policy replaces.  A lane of the adaptive
body walks until its last rule has stopped -- with a `never` rule in the list that is the whole pool -- and tests every open rule after
every sample, so the ratio shows the per-step price of the rule tests.

  python tools/adaptive_bench.py [--shapes a,b,c,d] [--reps 5] [--json out.json] [--resample-only]

Shapes (8 rules of cap N: never, margins 2 / 4 / 8, beta 0.9 / 0.95 / 0.99, never with SCV_STOP_DECIDED; synthetic peaked pools):
(a) P = 30, N = 128, R = 10^4 (the reference); (b) P = 10^4, N = 128, R = 10^3; (c) P = 10^4, N = 256, R = 256; (d) the pool order at
P = 10^5, N = 128 (next to the resample call at R = 1).  Kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call,
median of --reps.  --resample-only times the resample call alone: with SCV_LIB_PATH set to an older build of the library that is the
comparison at that build.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 10_000), "b": (10_000, 128, 1_000), "c": (10_000, 256, 256), "d": (100_000, 128, None)}
RULE_NAMES = ["never", "margin2", "margin4", "margin8", "beta0.90", "beta0.95", "beta0.99", "never+decided"]


def rules(N):
    import numpy as np
    from o1_inference_scaling_laws_amd.adaptive import STOP_DECIDED, beta_rule, margin_rule, never
    need = np.stack([never(N), margin_rule(N, 2), margin_rule(N, 4), margin_rule(N, 8), beta_rule(N, 0.9), beta_rule(N, 0.95),
                     beta_rule(N, 0.99), never(N)]).astype(np.int32)
    flags = np.array([0] * 7 + [STOP_DECIDED], dtype=np.int32)
    return np.full(8, N, dtype=np.int32), need, flags


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
    ap.add_argument("--resample-only", action="store_true")
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    out = {"rules": RULE_NAMES, "lib": os.environ.get("SCV_LIB_PATH") or "in-tree", "shapes": {}}
    with Engine(device=0, timing=True) as eng:
        dev = torch.device("cuda", eng.device)
        for key in args.shapes.split(","):
            P, N, R = SHAPES[key]
            pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tok = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tr = torch.empty((P,), dtype=torch.int32, device=dev)
            eng.synth_fill_device(pool, tok, tr, P=P, B=1, N=N, seed=7, dist=1)
            pool, tok = pool.view(P, N), tok.view(P, N)
            cap, need, flags = [torch.from_numpy(x).to(dev) for x in rules(N)]
            nv = torch.full((8,), N, dtype=torch.int32, device=dev)
            r_end = R if R is not None else None
            cells = P * (R or 1)
            row = {"P": P, "N": N, "R": R, "order": "shuffled" if R else "pool"}
            routs = eng.resample_prefix_device(pool, tr, nv, 0, R or 1, 1, tokens=tok)
            rbufs = dict(tie_class_hits=routs[0], token_sum=routs[1], truth_count_sum=routs[2])
            rs = timed(eng, lambda s: eng.resample_prefix_device(pool, tr, nv, 0, R or 1, s, tokens=tok, **rbufs), args.reps)
            row.update({"resample_n_eq_N_us": round(statistics.median(rs), 1), "resample_us_all": [round(x, 1) for x in rs]})
            if not args.resample_only:
                outs = eng.adaptive_prefix_device(pool, tr, cap, need, flags, tokens=tok, r_begin=0, r_end=r_end, seed=1)
                bufs = dict(tie_class_hits=outs[0], token_sum=outs[1], vote_count_sum=outs[2], truth_count_sum=outs[3], stop_hist=outs[4])
                ad = timed(eng, lambda s: eng.adaptive_prefix_device(pool, tr, cap, need, flags, tokens=tok, r_begin=0, r_end=r_end, seed=s,
                                                                     **bufs), args.reps)
                # what one call spent and scored, for the record
                one = eng.adaptive_prefix_device(pool, tr, cap, need, flags, tokens=tok, r_begin=0, r_end=r_end, seed=1)
                eng.sync()
                m = torch.arange(1, one[0].shape[1], dtype=torch.float64, device=dev)
                acc = (one[0][:, 1:].to(torch.float64) / m).sum(dim=1) / cells
                row.update({"avg_votes": [round(float(v) / cells, 2) for v in one[2].cpu().tolist()],
                            "avg_tokens_used": [round(float(v) / cells, 1) for v in one[1].cpu().tolist()],
                            "accuracy": [round(float(v), 4) for v in acc.cpu().tolist()],
                            "adaptive_us": round(statistics.median(ad), 1), "adaptive_us_all": [round(x, 1) for x in ad]})
                row["ratio"] = round(row["adaptive_us"] / row["resample_n_eq_N_us"], 3)
                del outs, one
            print(key, json.dumps(row), flush=True)
            out["shapes"][key] = row
            del pool, tok, tr, routs
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
