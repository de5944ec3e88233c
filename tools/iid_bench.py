#!/usr/bin/env python3
"""Timing of scv_iid_prefix_i32 (majority vote over draws with replacement, past the size of the pool) next to (a)
scv_resample_prefix_i32 with tokens at n_valid = N on the same pools -- the shuffle walk whose step this one is without the shuffle -- and
(b), at k <= 1024, the torch composition randint -> gather -> scv_aggregate_prefix_i32 on [P * R, k] rows.

  python tools/iid_bench.py [--shapes a,b,c] [--reps 5] [--json out.json] [--no-torch]

Shapes (synthetic peaked pools, D1, with tokens; draw budgets 1, 2, 4, ...): (a) P = 30, N = 128, R = 10^4, draws up to 128 (the
reference's grid); (b) the same pools, draws up to 4096; (c) P = 10^4, N = 128, R = 10^3, draws up to 128.  Kernel time from
SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call, median of --reps; the torch composition is timed with events around all of
it (it is several kernels, torch's among them) and only where its [P * R, k] index, vote and token tensors fit (shapes a and b; b at
k = 1024).  steps/s = P * R * max k / kernel time.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 10_000, 128, 128), "b": (30, 128, 10_000, 4096, 1024), "c": (10_000, 128, 1_000, 128, None)}     # P, N, R, max draws, torch k


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


def torch_composition(eng, pool, tok, tr, R, k, reps):
    """randint -> gather -> one vote per row of [P * R, k]: wall time between two events, microseconds."""
    import torch
    P, N = pool.shape
    dev = pool.device
    nv = torch.tensor([k], dtype=torch.int32, device=dev)
    trr = tr.repeat_interleave(R).contiguous()
    gen = torch.Generator(device=dev)

    def once(seed):
        gen.manual_seed(seed)
        idx = torch.randint(0, N, (P, R * k), device=dev, generator=gen)
        votes = torch.gather(pool, 1, idx).view(P * R, k)
        toks = torch.gather(tok, 1, idx).view(P * R, k)
        return eng.aggregate_prefix_device(votes, trr, nv, tokens=toks, cells=False)[0]
    once(0)
    eng.sync()
    out = []
    for rep in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        once(100 + rep)
        e1.record()
        eng.sync()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    eng.drain_kernel_ns()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    out = {"lib": os.environ.get("SCV_LIB_PATH") or "in-tree", "shapes": {}}
    with Engine(device=0, timing=True) as eng:
        dev = torch.device("cuda", eng.device)
        for key in args.shapes.split(","):
            P, N, R, kmax, ktorch = SHAPES[key]
            pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tok = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
            tr = torch.empty((P,), dtype=torch.int32, device=dev)
            eng.synth_fill_device(pool, tok, tr, P=P, B=1, N=N, seed=7, dist=1)
            pool, tok = pool.view(P, N), tok.view(P, N)
            draws = [1 << i for i in range(kmax.bit_length()) if (1 << i) <= kmax]
            nd = torch.tensor(draws, dtype=torch.int32, device=dev)
            nv = torch.full((8,), N, dtype=torch.int32, device=dev)
            cells = P * R
            row = {"P": P, "N": N, "R": R, "draws": draws}
            routs = eng.resample_prefix_device(pool, tr, nv, 0, R, 1, tokens=tok)
            rbufs = dict(tie_class_hits=routs[0], token_sum=routs[1], truth_count_sum=routs[2])
            rs = timed(eng, lambda s: eng.resample_prefix_device(pool, tr, nv, 0, R, s, tokens=tok, **rbufs), args.reps)
            row.update({"resample_n_eq_N_us": round(statistics.median(rs), 1), "resample_us_all": [round(x, 1) for x in rs]})
            outs = eng.iid_prefix_device(pool, tr, nd, 0, R, 1, tokens=tok)
            bufs = dict(tie_class_hits=outs[0], token_sum=outs[1], truth_count_sum=outs[2])
            ii = timed(eng, lambda s: eng.iid_prefix_device(pool, tr, nd, 0, R, s, tokens=tok, **bufs), args.reps)
            one = eng.iid_prefix_device(pool, tr, nd, 0, R, 1, tokens=tok)     # what one call scored, for the record
            whole = eng.aggregate_prefix_device(pool, tr, nv[:1].contiguous(), cells=False)[0]
            eng.sync()
            eng.drain_kernel_ns()
            m = torch.arange(1, one[0].shape[1], dtype=torch.float64, device=dev)
            acc = (one[0][:, 1:].to(torch.float64) / m).sum(dim=1) / cells
            limit = float((whole[1:1025].to(torch.float64) / m).sum() / P)
            us = statistics.median(ii)
            row.update({"iid_us": round(us, 1), "iid_us_all": [round(x, 1) for x in ii],
                        "accuracy": [round(float(v), 4) for v in acc.cpu().tolist()], "accuracy_whole_pool": round(limit, 4),
                        "avg_tokens_used": [round(float(v) / cells, 1) for v in one[1].cpu().tolist()],
                        "steps_per_s": float(f"{cells * kmax / (us * 1e-6):.4g}"),
                        "resample_steps_per_s": float(f"{cells * N / (row['resample_n_eq_N_us'] * 1e-6):.4g}")})
            row["step_cost_vs_shuffle"] = round((us / kmax) / (row["resample_n_eq_N_us"] / N), 3)
            del outs, one, routs
            if ktorch and not args.no_torch:
                try:
                    tt = torch_composition(eng, pool, tok, tr, R, ktorch, args.reps)
                except Exception as e:                                          # (out of memory, a refused shape: the row says so)
                    row["torch_error"] = str(e)[:200]
                    tt = None
            if ktorch and not args.no_torch and tt is not None:
                nk = torch.tensor([ktorch], dtype=torch.int32, device=dev)
                o1 = eng.iid_prefix_device(pool, tr, nk, 0, R, 1, tokens=tok)
                b1 = dict(tie_class_hits=o1[0], token_sum=o1[1], truth_count_sum=o1[2])
                i1 = timed(eng, lambda s: eng.iid_prefix_device(pool, tr, nk, 0, R, s, tokens=tok, **b1), args.reps)
                row.update({"torch_k": ktorch, "torch_composition_us": round(statistics.median(tt), 1), "torch_us_all": [round(x, 1) for x in tt],
                            "iid_one_budget_us": round(statistics.median(i1), 1)})
                row["torch_over_iid"] = round(row["torch_composition_us"] / row["iid_one_budget_us"], 1)
                del o1
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
