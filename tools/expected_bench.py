#!/usr/bin/env python3
"""Timing of scv_expected_majority_i32 (the exact expected majority vote over all k-subsets of a pool) against the sampled estimate
it replaces, scv_resample_prefix_i32 at R = 10^3 and 10^4, on the same pools.

  python tools/expected_bench.py [--shapes a,b,c] [--dists 1,0] [--reps 5] [--json out.json]

Shapes: (a) the reference, P = 30, N = 128, budgets 1, 2, 4 ... 128; (b) P = 10^4, N = 128, the same budgets; (c) P = 10^4, N = 256,
9 budgets (1 .. 256).  Distributions: synth D1 (peaked, AIME-like) and D0 (uniform: the most classes).  Kernel time from
SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call, median of --reps, the three calls alternated rep by rep.  FP64
operations are counted on the CPU from the kernel's work items (expected.item_fp64_ops: 2 per FMA of the factor products).  Run it
under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 8), "b": (10_000, 128, 8), "c": (10_000, 256, 9)}
FP64_VECTOR_PEAK = 78.6e12                   # MI355X: FP64 vector FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--dists", default="1,0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd import expected
    from o1_inference_scaling_laws_amd.engine import Engine
    out = {"fp64_vector_peak": FP64_VECTOR_PEAK, "shapes": {}}
    with Engine(device=0, timing=True) as eng:
        dev = torch.device("cuda", eng.device)
        for key in args.shapes.split(","):
            P, N, B = SHAPES[key]
            for dist in (int(d) for d in args.dists.split(",")):
                pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
                tr = torch.empty((P,), dtype=torch.int32, device=dev)
                eng.synth_fill_device(pool, None, tr, P=P, B=1, N=N, seed=7, dist=dist)
                pool = pool.view(P, N)
                nvl = [min(1 << k, N) for k in range(B)]
                nv = torch.tensor(nvl, dtype=torch.int32, device=dev)
                ph, th = pool.cpu().numpy(), tr.cpu().numpy()
                ops = 0
                for p in range(P):
                    ct, others = expected.row_classes(ph[p], int(th[p]))
                    ops += expected.item_fp64_ops(N, ct, others, max(nvl), hit=False)
                score = torch.empty((P, B), dtype=torch.float64, device=dev)
                calls = {"exact": lambda rep: eng.expected_majority_device(pool, tr, nv, score=score, want_hit_prob=False),
                         "resample_1e3": lambda rep: eng.resample_prefix_device(pool, tr, nv, 0, 1000, 100 + rep),
                         "resample_1e4": lambda rep: eng.resample_prefix_device(pool, tr, nv, 0, 10_000, 100 + rep)}
                times = {k: [] for k in calls}
                for k, f in calls.items():                                          # warm-up
                    f(0)
                eng.sync()
                eng.drain_kernel_ns()
                for rep in range(args.reps):
                    for k, f in calls.items():
                        f(rep)
                        eng.sync()
                        ns, n = eng.drain_kernel_ns()
                        times[k].append(ns / max(n, 1) / 1e3)
                row = {"P": P, "N": N, "B": B, "dist": dist, "budgets": nvl, "fp64_ops": ops}
                for k, ts in times.items():
                    row[k + "_us"] = round(statistics.median(ts), 1)
                    row[k + "_us_all"] = [round(x, 1) for x in ts]
                t = row["exact_us"] * 1e-6
                row["fp64_per_s"] = ops / t if t else None
                row["fp64_fraction_of_peak"] = ops / t / FP64_VECTOR_PEAK if t else None
                row["exact_accuracy"] = [float(v) for v in score.double().mean(dim=0).cpu()]
                print(key, f"D{dist}", json.dumps(row), flush=True)
                out["shapes"][f"{key}_D{dist}"] = row
                del pool, tr, score
                torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
