#!/usr/bin/env python3
"""Timing of scv_resample_wide_i32 (the expected majority vote over sorted random orderings of pools of up to 4096 samples) against what a
user does without it: torch rand(...).argsort -> gather the pool into [P * R, N] -> scv_aggregate_prefix_i32 (tools/resample_bench.py
``baseline``), on the same pools in the same run.  The two use different random numbers: the comparison is of time only.

  python tools/wide_bench.py [--shapes a,b,c,s128,s256] [--reps 5] [--no-baseline]
  python tools/wide_bench.py --siblings [--label parent] [--reps 5]

Shapes (D1 pools, budgets 1, 2, 4 ... N, with and without tokens): (a) P = 30, N = 1024, R = 10^3; (b) P = 30, N = 4096, R = 10^3;
(c) P = 10^3, N = 1024, R = 10^2; (s128 / s256) P = 30, N = 128 / 256, R = 10^3, also through scv_resample_prefix_i32: which entry to call
on small pools.  Kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call, median of --reps; the baseline is timed with
torch events over the same stream, alternating with the kernel rep by rep.  Every row carries the launch's workgroup size, LDS bytes and the
workgroups per CU that LDS allows (csrc/scvote_dispatch.h wide_lanes / wide_lds_words, restated here).
``--siblings``: the other bodies of scv_resample_prefix alone (tools/shortest_bench.py ``siblings`` and a short-m@k call), for A/B runs of
two builds of the library (SCV_LIB_PATH; --label names the build in the output).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)
sys.path.insert(0, os.path.join(R_, "tools"))

SHAPES = {"a": (30, 1024, 1_000), "b": (30, 4096, 1_000), "c": (1_000, 1024, 100), "s128": (30, 128, 1_000), "s256": (30, 256, 1_000)}
LDS_BYTES = 160 * 1024


# The geometry of the wide launches, csrc/scvote_dispatch.h restated ONCE for the tools (wide_open_bench.py and wide_budget_bench.py import
# it; tests/test_wide_budget_cpu.py holds it to the header).
def wide_pad(N):
    n2 = 2
    while n2 < N:
        n2 <<= 1
    return n2


def wide_lanes(N):
    return min(256, max(64, wide_pad(N) // 2))


def wide_hist_words(N, open_domain):
    return (max(1024, N) + 1) // 2 if open_domain else 1024


def wide_lds_words(N, B, open_domain=False):
    return 2 * wide_pad(N) + 4 * B + 16 + wide_hist_words(N, open_domain) + B * (min(N, 127) + 1) + 16 + 64 + (N + 1) // 2


def wide_budget_lds_words(N, B, open_domain=False):
    return 2 * wide_pad(N) + 6 * B + 64 + 8 + wide_hist_words(N, open_domain) + B * (min(N, 127) + 1) + 16 + 64 + (N + 1) // 2


def launch_shape(N, B):
    """(lanes, LDS bytes, workgroups per CU by LDS) of a wide launch."""
    lanes, lds = wide_lanes(N), 4 * wide_lds_words(N, B)
    return lanes, lds, min(LDS_BYTES // lds, 2048 // lanes, 32)


def timed(eng, fn, reps, between=None):
    fn(0)                                                                       # warm-up
    eng.sync()
    eng.drain_kernel_ns()
    out = []
    for rep in range(reps):
        fn(100 + rep)
        eng.sync()
        ns, n = eng.drain_kernel_ns()
        out.append(ns / max(n, 1) / 1e3)
        if between:
            between(rep)
    return out


def siblings(torch, Engine, reps, label):
    import shortest_bench
    shortest_bench.siblings(torch, Engine, reps, 128, label)
    from open_domain_bench import pools
    P, N, R = 30, 128, 10_000
    with Engine(device=0, timing=True) as eng:
        pool, tok, tr = pools(eng, torch, P, N)
        ks = [1 << i for i in range(N.bit_length())]
        nv = torch.tensor(ks, dtype=torch.int32, device=pool.device)
        mk = torch.tensor([(k + 3) // 4 for k in ks], dtype=torch.int32, device=pool.device)
        o = eng.shortest_prefix_device(pool, tok, tr, nv, mk, 0, R, 1)
        bufs = dict(tie_class_hits=o[0], voted_token_sum=o[1], spent_token_sum=o[2], latency_sum=o[3], truth_count_sum=o[4])
        us = timed(eng, lambda s: eng.shortest_prefix_device(pool, tok, tr, nv, mk, 0, R, s, **bufs), reps)
        print("sibling", "shortest", json.dumps({"P": P, "N": N, "R": R, "lib": label, "us": round(statistics.median(us), 1),
                                                 "us_all": [round(x, 1) for x in us]}), flush=True)
        big = pools(eng, torch, 2_000, N)                                       # the exact form: the workgroup-cooperative body of <false>
        s = eng.expected_majority_device(big[0], big[2], nv)
        us = timed(eng, lambda _s: eng.expected_majority_device(big[0], big[2], nv, score=s[0], hit_prob=s[1]), reps)
        print("sibling", "expected", json.dumps({"P": 2_000, "N": N, "R": None, "lib": label, "us": round(statistics.median(us), 1),
                                                 "us_all": [round(x, 1) for x in us]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,s128,s256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--siblings", action="store_true")
    ap.add_argument("--label", default="in-tree")
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    if args.siblings:
        siblings(torch, Engine, args.reps, args.label)
        return
    from resample_bench import baseline, pool_for
    with Engine(device=0, timing=True) as eng:
        for key in args.shapes.split(","):
            P, N, R = SHAPES[key]
            pool, tok, tr = pool_for(eng, P, N, 7)
            nvl = [1 << k for k in range(N.bit_length()) if (1 << k) <= N]
            nv = torch.tensor(nvl, dtype=torch.int32, device=pool.device)
            lanes, lds, per_cu = launch_shape(N, len(nvl))
            row = {"P": P, "N": N, "R": R, "B": len(nvl), "lanes": lanes, "lds_bytes": lds, "workgroups_per_cu_by_lds": per_cu,
                   "waves_per_cu": per_cu * lanes // 64}
            for tokens in (False, True):
                label = "tok" if tokens else "plain"
                t = tok if tokens else None
                o = eng.resample_wide_device(pool, tr, nv, 0, R, 1, tokens=t)
                bufs = dict(tie_class_hits=o[0], token_sum=o[1], truth_count_sum=o[2])
                bs = []

                def torch_composition(rep):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    baseline(eng, pool, tok, tr, nv, R, 100 + rep)
                    e1.record()
                    torch.cuda.synchronize()
                    eng.sync()
                    eng.drain_kernel_ns()
                    bs.append(e0.elapsed_time(e1) * 1e3)
                ws = timed(eng, lambda s: eng.resample_wide_device(pool, tr, nv, 0, R, s, tokens=t, **bufs), args.reps,
                           torch_composition if tokens and not args.no_baseline else None)
                w_us = statistics.median(ws)
                row[label] = {"wide_us": round(w_us, 1), "wide_us_all": [round(x, 1) for x in ws], "us_per_item": round(w_us / (P * R), 4)}
                if bs:
                    b_us = statistics.median(bs)
                    row[label].update({"argsort_gather_prefix_us": round(b_us, 1), "argsort_all_us": [round(x, 1) for x in bs],
                                       "torch_over_wide": round(b_us / w_us, 1)})
                if N <= 256:
                    ls = timed(eng, lambda s: eng.resample_prefix_device(pool, tr, nv, 0, R, s, tokens=t, **bufs), args.reps)
                    l_us = statistics.median(ls)
                    row[label].update({"resample_prefix_us": round(l_us, 1), "resample_prefix_us_all": [round(x, 1) for x in ls],
                                       "wide_over_resample_prefix": round(w_us / l_us, 2)})
            print(key, json.dumps(row), flush=True)
            del pool, tok, tr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
