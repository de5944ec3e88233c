#!/usr/bin/env python3
"""Timing of scv_weighted_prefix_i32 (weighted majority vote, rule 0, and best-of-N, rule 1, over the prefixes of pool orderings) next to
 * scv_resample_prefix_i32 on the same pools and budgets: the unweighted vote, the floor this body is not expected to beat (byte counts and
   codes in the Fisher-Yates array against uint32 totals per code); the ratio is reported, not fixed;
 * a torch composition on the GPU, what a user would write without the call: rand -> argsort -> gather votes and weights -> per budget (ascending,
   only the new samples) scatter_add / scatter_reduce(amax) into an [n, 1024] table -> max, count of modes, the truth's weight -> bincount.

  python tools/weighted_bench.py [--shapes a,b,c,d] [--reps 5] [--no-baseline] [--json out.json]

Shapes (D1 pools, weights 1 + mix64(7 + G (p N + i + 1)) % 1000; synthetic tokens): (a) the reference, P = 30,
N = 128, budgets 1, 2, 4 ... 128, R = 10^4; (b) P = 10^4, N = 128, the same budgets, R = 10^3; (c) P = 10^4, N = 256, 9 budgets (1 .. 256),
R = 256; (d) the pool order at P = 10^5, N = 128 (with cells).  Kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call,
median of --reps; the torch composition by device events around the whole composition, median of --baseline-reps.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 10_000), "b": (10_000, 128, 1_000), "c": (10_000, 256, 256), "d": (100_000, 128, None)}


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


def torch_composition(pool, w, tr, ks, R, rule, seed, max_rows=1 << 17):
    """tie classes [B, 1025] of the weighted vote over R random orderings per pool, in torch ops only."""
    import torch
    P, N = pool.shape
    dev = pool.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    order = sorted(range(len(ks)), key=lambda b: ks[b])
    tie = torch.zeros((len(ks), 1025), dtype=torch.int64, device=dev)
    rows = P * R
    w64 = w.to(torch.int64).reshape(-1)
    for r0 in range(0, rows, max_rows):
        n = min(max_rows, rows - r0)
        p_idx = torch.arange(r0, r0 + n, device=dev) // R
        perm = torch.rand((n, N), generator=gen, device=dev).argsort(dim=1)
        flat = (p_idx[:, None] * N + perm).reshape(-1)
        votes = pool.reshape(-1)[flat].view(n, N).to(torch.int64)
        ws = w64[flat].view(n, N)
        truth = tr[p_idx].to(torch.int64)[:, None]
        W = torch.zeros((n, 1024), dtype=torch.int64, device=dev)
        done = 0
        for b in order:
            k = ks[b]
            if k > done:
                if rule == 0:
                    W.scatter_add_(1, votes[:, done:k], ws[:, done:k])
                else:
                    W.scatter_reduce_(1, votes[:, done:k], ws[:, done:k], reduce="amax")
                done = k
            top = W.max(dim=1, keepdim=True).values
            nm = (W == top).sum(dim=1)
            tw = W.gather(1, truth)
            hit = ((tw == top) & (top > 0)).view(-1)
            tie[b] += torch.bincount(nm[hit], minlength=1025)[:1025]
    return tie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from o1_inference_scaling_laws_amd import synth
    from o1_inference_scaling_laws_amd.engine import Engine
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
            idx = np.arange(P * N, dtype=np.uint64)
            with np.errstate(over="ignore"):
                w = torch.from_numpy((1 + synth.mix64(np.uint64(7) + synth.G * (idx + np.uint64(1))) % np.uint64(1000)).astype(np.int32).reshape(P, N)).to(dev)
            ks = [1 << i for i in range(N.bit_length())]
            nv = torch.tensor(ks, dtype=torch.int32, device=dev)
            B = len(ks)
            r_end = R
            row = {"P": P, "N": N, "R": R, "budgets": ks, "order": "shuffled" if R else "pool"}
            tie = torch.zeros((B, 1025), dtype=torch.int64, device=dev)
            ts = torch.zeros((B,), dtype=torch.int64, device=dev)
            tcs = torch.zeros((B,), dtype=torch.int64, device=dev)
            for rule, name in ((0, "weight_sum"), (1, "best_of")):
                for with_tok in (False, True):
                    kw = dict(tokens=tok, token_sum=ts) if with_tok else {}
                    if R is None:
                        kw["want_cells"] = True
                    us = timed(eng, lambda s: eng.weighted_prefix_device(pool, w, tr, nv, rule, 0, r_end, s, tie_class_hits=tie, **kw), args.reps)
                    label = name + ("_tok" if with_tok else "")
                    row[label + "_us"] = round(statistics.median(us), 1)
                    row[label + "_us_all"] = [round(x, 1) for x in us]
            for with_tok in (False, True):
                kw = dict(tokens=tok, token_sum=ts) if with_tok else {}
                rs = timed(eng, lambda s: eng.resample_prefix_device(pool, tr, nv, 0, R or 1, s, tie_class_hits=tie, truth_count_sum=tcs, **kw),
                           args.reps)
                label = "resample" + ("_tok" if with_tok else "")
                row[label + "_us"] = round(statistics.median(rs), 1)
                row[label + "_us_all"] = [round(x, 1) for x in rs]
            row["weight_sum_over_resample"] = round(row["weight_sum_us"] / row["resample_us"], 2)
            row["weight_sum_tok_over_resample_tok"] = round(row["weight_sum_tok_us"] / row["resample_tok_us"], 2)
            if not args.no_baseline and R is not None:
                for rule, name in ((0, "weight_sum"), (1, "best_of")):
                    ms = []
                    for rep in range(args.baseline_reps + 1):
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        torch_composition(pool, w, tr, ks, R, rule, 100 + rep)
                        e1.record()
                        torch.cuda.synchronize()
                        if rep:
                            ms.append(e0.elapsed_time(e1) * 1e3)
                    row["torch_" + name + "_us"] = round(statistics.median(ms), 1)
                    row["torch_" + name + "_us_all"] = [round(x, 1) for x in ms]
                    row["torch_over_" + name] = round(row["torch_" + name + "_us"] / row[name + "_us"], 1)
            print(key, json.dumps(row), flush=True)
            out["shapes"][key] = row
            del pool, tok, tr, w
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
