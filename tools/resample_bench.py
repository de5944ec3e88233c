#!/usr/bin/env python3
"""Timing of scv_resample_prefix_i32 (the expected majority vote over random pool orderings) against what a user does without it:
torch rand(...).argsort -> gather the pool into [P * R, N] -> scv_aggregate_prefix_i32.  The two use different random numbers, so
the comparison is of time only (both produce P * R cells per budget).

  python tools/resample_bench.py [--shapes a,b,c] [--reps 5] [--no-baseline] [--json out.json]
  python tools/resample_bench.py --isa          # VALU instructions per shuffle step from the gfx950 ISA (no GPU)

Shapes: (a) the reference, P = 30, N = 128, budgets 1, 2, 4 ... 128, R = 10^4; (b) P = 10^4, N = 128, the same budgets, R = 10^3;
(c) P = 10^4, N = 256, 9 budgets (1 .. 256), R = 256.  Kernel time from SCV_FLAG_TIMING (scv_drain_kernel_ns) after one warm-up call,
median of --reps; the baseline is timed with torch events over the same stream, alternating with the kernel rep by rep.  Run it
under `timeout`; a kernel-level trace is a separate run under `rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py`."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)

SHAPES = {"a": (30, 128, 8, 10_000), "b": (10_000, 128, 8, 1_000), "c": (10_000, 256, 9, 256)}
VALU_PEAK_LANE_OPS = 157.3e12 / 2           # MI355X_MICROARCH: 157.3 TFLOPS FP32 vector = FMA lane-ops x 2


def isa_valu_per_step():
    """Instructions of one shuffle step of each instantiation, from the gfx950 ISA: the cheapest path (fewest instructions) from the
    header of the step loop -- the loop whose header holds mix64's first 64-bit shift -- back to it, i.e. a step that crosses no budget
    boundary (a boundary adds the DPP reductions and table atomics once per budget, not per step)."""
    import heapq
    src = os.path.join(R_, "o1_inference_scaling_laws_amd", "csrc", "scvote_resample.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        s = open(out).read()
    res = {}
    for m in re.finditer(r"^(_ZN3scv19scv_resample_prefixILb([01])EE\w*):\s*(;.*)?$", s, re.M):
        body = s[m.end():s.index("s_endpgm", m.end())]
        blocks, cur, name = [], [], "entry"
        for line in body.splitlines():
            t = line.strip()
            lab = re.match(r"^(\.LBB\w+):", t) or re.match(r"^; (%bb\.\d+):", t)
            if lab:
                blocks.append((name, cur))
                name, cur = lab.group(1), []
                continue
            if t and not t.startswith((";", ".")):
                cur.append(t.split(";")[0].strip())
        blocks.append((name, cur))
        index = {n: i for i, (n, _) in enumerate(blocks)}
        back = {x.split()[1]: j for j, (_n, b) in enumerate(blocks) for x in b if x.startswith(("s_cbranch", "s_branch"))}
        head = next((i for i, (n, b) in enumerate(blocks) if back.get(n, -1) >= i and any(re.match(r"v_lshrrev_b64 \S+, 30,", y) for y in b)), None)
        if head is None:
            continue

        def succ(i):
            b = blocks[i][1]
            last = b[-1].split() if b else []
            out_ = [index[last[1]]] if last and last[0] == "s_branch" else ([i + 1] if i + 1 < len(blocks) else [])
            return out_ + [index[x.split()[1]] for x in b if x.startswith("s_cbranch") and x.split()[1] in index]
        dist, prev, heap = {head: len(blocks[head][1])}, {}, [(len(blocks[head][1]), head)]
        found = None
        while heap:
            dd, i = heapq.heappop(heap)
            if dd > dist.get(i, 1 << 30):
                continue
            for j in succ(i):
                if j == head:
                    found = i
                    break
                nd = dd + len(blocks[j][1])
                if nd < dist.get(j, 1 << 30):
                    dist[j], prev[j] = nd, i
                    heapq.heappush(heap, (nd, j))
            if found is not None:
                break
        path, i = [], found
        while i is not None:
            path.append(i)
            i = prev.get(i)
        step = [y.split()[0] for i in path for y in blocks[i][1]]
        res["tok" if m.group(2) == "1" else "plain"] = {
            "valu": sum(1 for y in step if y.startswith("v_")),
            "lds": sum(1 for y in step if y.startswith("ds_")),
            "salu": sum(1 for y in step if y.startswith("s_") and y not in ("s_nop", "s_waitcnt")),
            "vmem": sum(1 for y in step if y.startswith(("global_", "buffer_", "flat_")))}
    return res


def pool_for(eng, P, N, seed):
    import torch
    dev = torch.device("cuda", eng.device)
    pool = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
    tok = torch.empty((P, 1, N), dtype=torch.int32, device=dev)
    tr = torch.empty((P,), dtype=torch.int32, device=dev)
    eng.synth_fill_device(pool, tok, tr, P=P, B=1, N=N, seed=seed, dist=1)
    return pool.view(P, N), tok.view(P, N), tr


def baseline(eng, pool, tok, tr, nv, R, seed, max_elems=1 << 28):
    """rand -> argsort -> gather -> one prefix call over [P * R, N] (chunked by rows so that one chunk's tensors stay ~4 GiB)."""
    import torch
    P, N = pool.shape
    gen = torch.Generator(device=pool.device)
    gen.manual_seed(seed)
    B = nv.shape[0]
    from o1_inference_scaling_laws_amd.engine import counters_size
    counters = torch.zeros(counters_size(B), dtype=torch.int64, device=pool.device)
    rows = P * R
    step = max(R, (max_elems // N) // R * R)
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        p_idx = torch.arange(r0, r0 + n, device=pool.device) // R
        perm = torch.rand((n, N), generator=gen, device=pool.device).argsort(dim=1)
        flat = (p_idx[:, None] * N + perm).reshape(-1)
        votes = pool.reshape(-1)[flat].view(n, N)
        toks = tok.reshape(-1)[flat].view(n, N)
        eng.aggregate_prefix_device(votes, tr[p_idx].contiguous(), nv, tokens=toks, counters=counters, cells=False)
    return counters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--isa", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    isa = isa_valu_per_step()
    print("ISA per shuffle step:", json.dumps(isa), flush=True)
    if args.isa:
        return
    import statistics
    import torch
    from o1_inference_scaling_laws_amd.engine import Engine
    out = {"isa_per_step": isa, "valu_peak_lane_ops_per_s": VALU_PEAK_LANE_OPS, "shapes": {}}
    with Engine(device=0, timing=True) as eng:
        for key in args.shapes.split(","):
            P, N, B, R = SHAPES[key]
            pool, tok, tr = pool_for(eng, P, N, 7)
            nvl = [min(1 << k, N) for k in range(B)]
            nv = torch.tensor(nvl, dtype=torch.int32, device=pool.device)
            kmax = max(nvl)
            steps = P * R * kmax
            row = {"P": P, "N": N, "B": B, "R": R, "budgets": nvl, "steps": steps}
            for tokens in (False, True):
                label = "tok" if tokens else "plain"
                eng.resample_prefix_device(pool, tr, nv, 0, R, 1, tokens=tok if tokens else None)      # warm-up
                eng.sync()
                eng.drain_kernel_ns()
                ks, bs = [], []
                for rep in range(args.reps):
                    eng.resample_prefix_device(pool, tr, nv, 0, R, 100 + rep, tokens=tok if tokens else None)
                    eng.sync()
                    ns, n = eng.drain_kernel_ns()
                    ks.append(ns / max(n, 1) / 1e3)
                    if tokens and not args.no_baseline:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        baseline(eng, pool, tok, tr, nv, R, 100 + rep)
                        e1.record()
                        torch.cuda.synchronize()
                        eng.sync()
                        eng.drain_kernel_ns()
                        bs.append(e0.elapsed_time(e1) * 1e3)
                k_us = statistics.median(ks)
                v = isa.get(label, {}).get("valu")
                row[label] = {"kernel_us": round(k_us, 1), "kernel_us_all": [round(x, 1) for x in ks],
                              "steps_per_s": steps / (k_us * 1e-6),
                              "valu_per_step_isa": v,
                              "valu_fraction_of_peak": (steps * v / (k_us * 1e-6)) / VALU_PEAK_LANE_OPS if v else None}
                if bs:
                    b_us = statistics.median(bs)
                    row[label].update({"argsort_gather_prefix_us": round(b_us, 1), "argsort_all_us": [round(x, 1) for x in bs],
                                       "speedup": round(b_us / k_us, 1)})
                print(key, label, json.dumps(row[label]), flush=True)
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
