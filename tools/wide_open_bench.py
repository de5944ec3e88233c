#!/usr/bin/env python3
"""Timing of scv_resample_wide_i32 on a SCV_FLAG_OPEN_DOMAIN context against a flag-off context, the two alternating rep by rep on the
same D1 pools (values inside 0..1023: both contexts compute the same bits).  What the flag adds is one row encoding -- a second sort -- per
problem of a workgroup's run; what it takes away is the scan of 1024 bins per budget (it scans the row's D distinct values).

  python tools/wide_open_bench.py [--shapes a,b,c,r1,d4096] [--reps 5]
  python tools/wide_open_bench.py --siblings [--label parent] [--reps 5]

Shapes (budgets 1, 2, 4 ... N, with tokens): (a) P = 30, N = 1024, R = 10^3; (b) P = 30, N = 4096, R = 10^3; (c) P = 10^3, N = 1024,
R = 10^2 (tools/wide_bench.py's); (r1) P = 10^4, N = 1024, R = 1: every item pays the encoder; (d4096) P = 30, N = 4096, R = 10^3 on a pool
of 32-bit values with more than 1024 distinct ones per row, which only the flag-on context can take.  Kernel time from SCV_FLAG_TIMING after
one warm-up call, median of --reps.  Every row carries the LDS bytes and the workgroups per CU of the two launches
(csrc/scvote_dispatch.h wide_lds_words, restated in tools/wide_bench.py).
``--siblings``: the flag-off wide call and the shuffle, weighted and draws-with-replacement bodies (N = 128) alone, for A/B runs of two
builds of the library (SCV_LIB_PATH; --label names the build in the output).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)
sys.path.insert(0, os.path.join(R_, "tools"))

SHAPES = {"a": (30, 1024, 1_000), "b": (30, 4096, 1_000), "c": (1_000, 1024, 100), "r1": (10_000, 1024, 1), "d4096": (30, 4096, 1_000)}
LDS_BYTES = 160 * 1024


def launch_shape(N, B, open_domain):
    """(lanes, LDS bytes, workgroups per CU) of a wide launch (the geometry: tools/wide_bench.py)."""
    from wide_bench import wide_lanes, wide_lds_words
    lanes, lds = wide_lanes(N), 4 * wide_lds_words(N, B, open_domain)
    return lanes, lds, min(LDS_BYTES // lds, 28 * 64 // lanes, 32)                        # 7 waves per SIMD: 28 per CU


def timed_pair(engs, fns, reps):
    """Median kernel time [us] of each (engine, call), the calls alternating rep by rep."""
    out = [[] for _ in engs]
    for eng, fn in zip(engs, fns):
        if fn:
            fn(0)                                                               # warm-up
            eng.sync()
            eng.drain_kernel_ns()
    for rep in range(reps):
        for i, (eng, fn) in enumerate(zip(engs, fns)):
            if fn:
                fn(100 + rep)
                eng.sync()
                ns, n = eng.drain_kernel_ns()
                out[i].append(ns / max(n, 1) / 1e3)
    return out


def siblings(torch, Engine, reps, label):
    from open_domain_bench import call_of, pools
    from resample_bench import pool_for
    with Engine(device=0, timing=True) as eng:
        P, N, R = SHAPES["a"]
        pool, tok, tr = pool_for(eng, P, N, 7)
        nv = torch.tensor([1 << k for k in range(N.bit_length())], dtype=torch.int32, device=pool.device)
        o = eng.resample_wide_device(pool, tr, nv, 0, R, 1, tokens=tok)
        calls = {"wide_flag_off": (P, N, R, lambda s: eng.resample_wide_device(pool, tr, nv, 0, R, s, tokens=tok, tie_class_hits=o[0],
                                                                               token_sum=o[1], truth_count_sum=o[2]))}
        P2, N2, R2 = 30, 128, 10_000
        small = pools(eng, torch, P2, N2)
        nv2 = torch.tensor([1 << i for i in range(N2.bit_length())], dtype=torch.int32, device=pool.device)
        o2 = eng.iid_prefix_device(small[0], small[2], nv2, 0, R2, 1, tokens=small[1])
        calls["shuffle"] = (P2, N2, R2, call_of(eng, torch, "resample", *small, R2))
        calls["weighted"] = (P2, N2, R2, call_of(eng, torch, "weighted", *small, R2))
        calls["iid"] = (P2, N2, R2, lambda s: eng.iid_prefix_device(small[0], small[2], nv2, 0, R2, s, tokens=small[1], tie_class_hits=o2[0],
                                                                     token_sum=o2[1], truth_count_sum=o2[2]))
        for kind, (p, n, r, fn) in calls.items():
            us, = timed_pair([eng], [fn], reps)
            print("sibling", kind, json.dumps({"P": p, "N": n, "R": r, "lib": label, "us": round(statistics.median(us), 1),
                                               "us_all": [round(x, 1) for x in us]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,r1,d4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--siblings", action="store_true")
    ap.add_argument("--label", default="in-tree")
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    if args.siblings:
        siblings(torch, Engine, args.reps, args.label)
        return
    from resample_bench import pool_for
    with Engine(device=0, timing=True, open_domain=True) as on, Engine(device=0, timing=True) as off:
        for key in args.shapes.split(","):
            P, N, R = SHAPES[key]
            pool, tok, tr = pool_for(off, P, N, 7)
            distinct = None
            if key == "d4096":                                                  # a peak at the truth, the rest 32-bit hashes: D > 1024 in every row
                g = torch.Generator(device=pool.device)
                g.manual_seed(11)
                noise = torch.randint(-2 ** 31, 2 ** 31 - 1, pool.shape, dtype=torch.int64, device=pool.device, generator=g).to(torch.int32)
                keep = torch.rand(pool.shape, device=pool.device, generator=g) < 0.3
                pool = torch.where(keep, (tr * 1_000_003 - 7)[:, None], noise).contiguous()
                tr = (tr * 1_000_003 - 7).contiguous()
                distinct = [int(torch.unique(pool[p]).numel()) for p in range(min(P, 4))]
            nvl = [1 << k for k in range(N.bit_length()) if (1 << k) <= N]
            nv = torch.tensor(nvl, dtype=torch.int32, device=pool.device)
            row = {"P": P, "N": N, "R": R, "B": len(nvl)}
            for name, flag in (("on", True), ("off", False)):
                lanes, lds, per_cu = launch_shape(N, len(nvl), flag)
                row[name + "_launch"] = {"lanes": lanes, "lds_bytes": lds, "workgroups_per_cu": per_cu}
            if distinct:
                row["distinct_in_first_rows"] = distinct
            fns = []
            for eng in (on, off):
                if eng is off and key == "d4096":
                    fns.append(None)
                    continue
                o = eng.resample_wide_device(pool, tr, nv, 0, R, 1, tokens=tok)
                fns.append(lambda s, eng=eng, o=o: eng.resample_wide_device(pool, tr, nv, 0, R, s, tokens=tok, tie_class_hits=o[0],
                                                                            token_sum=o[1], truth_count_sum=o[2]))
            us_on, us_off = timed_pair([on, off], fns, args.reps)
            row["on_us"] = round(statistics.median(us_on), 1)
            row["on_us_all"] = [round(x, 1) for x in us_on]
            if us_off:
                row["off_us"] = round(statistics.median(us_off), 1)
                row["off_us_all"] = [round(x, 1) for x in us_off]
                row["on_over_off"] = round(statistics.median(us_on) / statistics.median(us_off), 3)
            print(key, json.dumps(row), flush=True)
            del pool, tok, tr, fns
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
