"""Guard bands around the outputs of DEVICE-mode scv_aggregate_i32 / scv_aggregate_prefix_i32.

``draw(seed)`` returns one complete, valid DEVICE-mode call that depends on the seed alone: the stratum is ``STRATA[seed % len(STRATA)]`` (each at
the smallest size where that kernel's store pattern has a ragged end), everything else -- tokens, n_valid, cell table wanted or not, 16-byte or
packed records, overwrite or accumulation, the alignment class of every tensor -- comes from ``default_rng((STREAM, seed))``.  ``layout(case)``
carves every tensor of the call out of ONE byte arena with at least GUARD bytes before, between and behind them, ``host_arena`` fills it (inputs,
previous counters, a byte pattern over every output and output guard, out-of-domain int32 values over the input guards), ``expected_arena``
writes what oracle.coracle says the call leaves behind, and ``check`` compares the whole arena byte for byte -- so one comparison covers the guard
bands, the inputs, the regions nobody asked for and the results.  ``plan_queries`` / ``plan_of`` ask tests/plan_check.cpp which kernel a draw reaches.

No GPU and no torch at module level: tests/test_agg_guard_cpu.py proves the reach and that the checker catches planted faults,
tests/test_gpu_agg_guard.py holds the kernels to it.  Nothing here has a tolerance: every comparison is exact."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import coracle

STREAM = 7_300_000
GUARD = 256                                   # bytes before, between and behind the tensors (at least)
PATTERN = 0xA5                                # outputs, output guards, regions nobody asked for
INPUT_GUARD = 0x7F                            # input guards: int32 0x7f7f7f7f -- outside the vote domain, a huge token count
TIE_CLASSES = 1025
CELL_ALIGN, CTOK_ALIGN, COUNTER_ALIGN = 16, 16, 8      # the widest store each output receives (include/scvote.h)
OPTION_DEFAULTS = (("path", 0), ("segs", 0), ("grid", 0), ("fused_counters_max", 512), ("reg_n_max", 8192), ("reg_shape", 0), ("prefix_path", 0),
                   ("sort_n_min", 8), ("sort_n_max", 64))
SPARSE_SHAPES = {1601: 64, 1602: 128, 1604: 256, 3204: 512, 6404: 1024}        # code -> slots (4 * g * v)
DENSE_SHAPES = {1041: 1024, 1042: 2048, 1044: 4096, 1048: 8192}


# ---- strata: (name, builder(rng) -> dict) ------------------------------------------------------------------------------------------------------

def _split_cells(rng, ncells, bmax=40):
    """(P, B) with P * B == ncells, B a random divisor of ncells up to bmax."""
    divs = [b for b in range(1, min(bmax, ncells) + 1) if ncells % b == 0]
    B = int(rng.choice(divs))
    return ncells // B, B


def _dense(P, B, N, aligned=False, packable=True, **opts):
    return dict(prefix=False, P=P, B=B, N=N, aligned=aligned, packable=packable and N <= 127, opts=opts)


def _prefix(P, N, budgets, aligned=False, host=False, **opts):
    return dict(prefix=True, P=P, B=len(budgets), N=N, aligned=aligned, packable=False, opts=opts, budgets=[int(b) for b in budgets], budgets_host=host)


def _few_big(N):
    def f(rng):                                # above 65536 cells, no multiple of 256 / N: scv_one_vote / scv_two_votes take the tail themselves
        B = int(rng.choice([1, 3, 8]))
        P = (65536 + int(rng.integers(1, 700))) // B + 1
        while (P * B) % (256 // N) == 0:
            P += 1
        return _dense(P, B, N, aligned=True)
    return f


def _few_small(N):
    def f(rng):                                # below 65536 cells, ragged: the general one-lane-per-cell kernel takes the call
        ncells = int(rng.choice([1, 255, 257, 1000, 4099]))
        return _dense(*_split_cells(rng, ncells, 12), N, aligned=True)
    return f


def _few_whole(N):
    def f(rng):                                # whole blocks; grids that are multiples of B and grids that are not; the grid forced below B
        B = int(rng.choice([1, 2, 4, 3, 11, 19]))
        P = (256 // N) * int(rng.choice([1, 3, 16, 17]))
        grid = int(rng.choice([0, 0, 1, 2, 3, 7]))
        return _dense(P, B, N, aligned=True, grid=grid)
    return f


def _lane(N):
    def f(rng):                                # one lane per cell, the sort off: 1, 63, 65, 1024 k + 1 cells
        ncells = int(rng.choice([1, 63, 65, 1025, 2049]))
        return _dense(*_split_cells(rng, ncells), N, sort_n_max=0)
    return f


def _sorted(nv):
    def f(rng):                                # every sort_nv shape: 1 and 64 k +- 1 cells; B that divides the wave step of 64 cells and B that does not
        N = int(rng.choice([nv, nv - 1, nv - 3]))
        ncells = int(rng.choice([1, 63, 65, 127, 129, 321]))
        return _dense(*_split_cells(rng, ncells), N, path=5)
    return f


def _sorted_b(rng):
    B = int(rng.choice([2, 4, 8, 64, 3, 7]))
    return _dense(int(rng.choice([16, 17, 33])), B, int(rng.choice([12, 30, 64])))


def _reg(code, slots):
    def f(rng, visit):                         # forced register shape: N at the capacity (aligned rows), at capacity - 3 (unaligned rows: N + 3 slots),
        back = (0, 3, 4, 1, 0, 3)[visit % 6]                           # capacity - 4, and capacity - 1 (one slot too many: the shape is ignored)
        ncells = int(rng.choice([1, 7, 67] if slots <= 1024 else [1, 5]))
        return _dense(*_split_cells(rng, ncells, 7), slots - back, aligned=back == 0, path=4, reg_shape=code)
    f.by_visit = True                          # (the stratum's visit number, seed // len(STRATA), picks the variant: every one within six seeds)
    return f


def _reg_auto(votes):                          # the auto shapes of 65 .. 96 / 97 .. 128 slots (8 lanes per cell, 3 / 4 vectors)
    def f(rng):
        return _dense(*_split_cells(rng, int(rng.choice([1, 9, 67])), 7), int(rng.choice(votes)), aligned=True, path=4)
    return f


def _stream_whole(rng):                        # path 1: P * B of 1 and of a few
    P, B = [(1, 1), (1, 1), (3, 1), (2, 2), (1, 5)][int(rng.integers(0, 5))]
    return _dense(P, B, int(rng.choice([100, 127, 5000, 70001])), packable=False, path=1)


def _stream_split(rng):                        # path 2 with 3 segments at N = 5000
    P, B = [(1, 1), (2, 1), (1, 3)][int(rng.integers(0, 3))]
    return _dense(P, B, 5000, packable=False, path=2, segs=3)


def _stream_dispenser(rng):                    # the item dispenser: 2 workgroups, three cells of 2^20 votes
    return _dense(3, 1, 1 << 20, aligned=True, packable=False, path=1, grid=2)


def _stream_reduce(rng, visit):                # counters out of the cell table (scv_reduce_cells) and inside the launch
    d = _dense(int(rng.choice([2, 3, 5])), int(rng.choice([1, 2])), int(rng.choice([9000, 9001])), packable=False, fused_counters_max=visit & 1)
    d["overwrite"] = visit % 3 == 2                     # (overwriting few cells happens inside the launch: no reduce launch)
    return d


_stream_reduce.by_visit = True


def _pow2(N, whole):
    cap = 16 if N <= 32 else (32 if N <= 64 else 64)
    b = [1 << k for k in range(7) if (1 << k) <= cap and (1 << k) <= N]
    return b + ([N] if whole else [])


def _p(rng):
    return int(rng.choice([1, 63, 257, 1100]))


def _sort_prefix(N):
    def f(rng):                                # budgets out of one sort per problem; pools above 64 only when the caller promises the list
        host = bool(rng.integers(0, 2)) or N > 64
        return _prefix(_p(rng), N, _pow2(N, bool(rng.integers(0, 2))), aligned=True, host=host)
    return f


def _lane_prefix(rng):
    N = int(rng.choice([1, 7, 16, 33, 64]))
    return _prefix(_p(rng), N, _budget_list(rng, N, int(rng.integers(1, 9))), prefix_path=1)


def _prefix_pool(rng):
    N = int(rng.choice([65, 1025]))
    return _prefix(int(rng.choice([1, 5, 63] if N > 65 else [1, 63, 257])), N, _budget_list(rng, N, int(rng.integers(1, 7))))


def _prefix_cells(rng):
    N = int(rng.choice([24, 200]))
    return _prefix(int(rng.choice([1, 63, 257])), N, _budget_list(rng, N, int(rng.integers(1, 6))), prefix_path=2)


def _prefix_hist(rng):
    N = int(rng.choice([4999, 5000]))
    return _prefix(int(rng.choice([1, 3])), N, _budget_list(rng, N, int(rng.integers(1, 5))))


def _budget_list(rng, N, B):
    edges = [0, 1, max(N - 1, 0), N, N + 1]
    return [int(rng.choice(edges)) if rng.random() < 0.6 else int(rng.integers(0, N + 2)) for _ in range(B)]


STRATA = ([(f"few_big_{n}", _few_big(n)) for n in (1, 2)] + [(f"few_small_{n}", _few_small(n)) for n in (1, 2, 4)] +
          [(f"few_whole_{n}", _few_whole(n)) for n in (1, 2, 4)] + [(f"lane_{n}", _lane(n)) for n in (3, 5, 8, 16, 32)] +
          [(f"sorted_{nv}", _sorted(nv)) for nv in range(8, 65, 8)] + [("sorted_b", _sorted_b)] +
          [(f"reg_{c}", _reg(c, s)) for c, s in {**SPARSE_SHAPES, **DENSE_SHAPES}.items()] + [("reg_auto_803", _reg_auto([65, 68, 93, 96])), ("reg_auto_804", _reg_auto([97, 100, 125, 128]))] +
          [("stream_whole", _stream_whole), ("stream_split", _stream_split), ("stream_dispenser", _stream_dispenser), ("stream_reduce", _stream_reduce)] +
          [(f"sort_prefix_{n}", _sort_prefix(n)) for n in (20, 32, 36, 64, 68, 128)] +
          [("lane_prefix", _lane_prefix), ("prefix_pool", _prefix_pool), ("prefix_cells", _prefix_cells), ("prefix_hist", _prefix_hist)])
DEFAULT_SEEDS = 6 * len(STRATA)                # seeds tests/test_gpu_agg_guard.py runs and tests/test_agg_guard_cpu.py proves the reach on


def draw(seed: int):
    name, build = STRATA[seed % len(STRATA)]
    rng = np.random.default_rng((STREAM, seed))
    made = build(rng, seed // len(STRATA)) if getattr(build, "by_visit", False) else build(rng)
    c = SimpleNamespace(**{"seed": seed, "stratum": name, "budgets": None, "budgets_host": False, **made})
    P, B, N = c.P, c.B, c.N
    c.tokens_on = bool(rng.integers(0, 2))
    c.want_cells = bool(rng.random() < 0.7)
    c.packed = bool(c.packable and c.want_cells and rng.integers(0, 2))
    c.overwrite = bool(rng.integers(0, 2)) if getattr(c, "overwrite", None) is None else c.overwrite
    c.ctok_given = bool(c.tokens_on and (c.want_cells or rng.integers(0, 2))) or bool(not c.tokens_on and rng.integers(0, 2))
    # the data: every distribution of the synthetic generator, folded into few bins on a third of the draws (heavy ties)
    dist = int(rng.integers(0, 6))
    a, t, tr = coracle.synth_fill(P, 1 if c.prefix else B, N, 60_000 + seed, dist, want_tokens=True)
    if rng.random() < 0.35:
        fold = int(rng.choice([2, 3, 5]))
        a, tr = (a % fold).astype(np.int32), (tr % fold).astype(np.int32)
    if rng.random() < 0.3:
        tr[:: int(rng.integers(1, 5))] = int(rng.choice([1023, -3, 2000]))
    c.votes = np.ascontiguousarray(a[:, 0, :] if c.prefix else a)
    c.tokens = np.ascontiguousarray(t[:, 0, :] if c.prefix else t) if c.tokens_on else None
    c.truth = tr.astype(np.int32)
    if c.prefix:
        c.n_valid = np.array(c.budgets, dtype=np.int32)
    elif rng.random() < 0.4:
        c.n_valid = None
    else:                                      # ragged, with 0, 1, N - 1, N and N + 1 in it
        c.n_valid = np.array(_budget_list(rng, N, B), dtype=np.int32)
    c.prev = rng.integers(0, 1 << 40, size=counters_size(B)).astype(np.int64)      # accumulate: onto these; overwrite: dirt
    # alignment classes: the vote and token bases over all four classes mod 16 unless the stratum's kernel needs aligned rows; the cell tables at
    # an odd multiple of 16 and the counters at an odd multiple of 8 on half the draws -- the documented alignment and nothing more
    c.align = {"votes": 0 if c.aligned else 4 * int(rng.integers(0, 4)), "tokens": 0 if c.aligned else 4 * int(rng.integers(0, 4)),
               "truth": 4 * int(rng.integers(0, 4)), "n_valid": 4 * int(rng.integers(0, 4)),
               "cells": 16 * int(rng.integers(0, 2)), "cell_tokens": 16 * int(rng.integers(0, 2)), "counters": 8 * int(rng.integers(0, 2))}
    return c


def counters_size(B):
    return B * TIE_CLASSES + 2 * B


def rows_aligned(c):
    return c.N % 4 == 0 and c.align["votes"] == 0 and (not c.tokens_on or c.align["tokens"] == 0)


# ---- the arena -----------------------------------------------------------------------------------------------------------------------------------

INPUTS, OUTPUTS = ("votes", "tokens", "truth", "n_valid"), ("counters", "cells", "cell_tokens")


def layout(c):
    """name -> (offset, nbytes) inside the arena (whose base is 256-byte aligned), and the arena's size.  A region is there whether the call asks
    for it or not; offset % 32 == its alignment class (so a class of 16 is an ODD multiple of 16, a class of 8 an odd multiple of 8)."""
    ncells = c.P * c.B
    sizes = {"votes": 4 * c.votes.size, "tokens": 4 * c.votes.size, "truth": 4 * c.P, "n_valid": 4 * c.B, "counters": 8 * counters_size(c.B),
             "cells": (4 if c.packed else 16) * ncells, "cell_tokens": 8 * ncells}
    regions, off = {}, 0
    for name in ("votes", "cells", "tokens", "counters", "truth", "cell_tokens", "n_valid"):       # inputs and outputs interleaved
        off += GUARD
        off = (off + 31) // 32 * 32 + c.align[name]
        regions[name] = (off, sizes[name])
        off += sizes[name]
    return regions, (off + GUARD + 31) // 32 * 32


def requested(c):
    """The outputs the call passes to the library."""
    return {"counters": True, "cells": c.want_cells, "cell_tokens": c.ctok_given}


def host_arena(c, regions, size):
    arena = np.full(size, PATTERN, dtype=np.uint8)
    ends = sorted((o, o + n, name) for name, (o, n) in regions.items())
    for i, (o, e, name) in enumerate(ends):                       # the guards on both sides of an input hold out-of-domain int32 values
        if name in INPUTS:
            lo = ends[i - 1][1] if i else 0
            hi = ends[i + 1][0] if i + 1 < len(ends) else size
            before, after = min(GUARD // 2, o - lo), min(GUARD // 2, hi - e)
            arena[o - before:o] = INPUT_GUARD
            arena[e:e + after] = INPUT_GUARD
            arena[o:e] = INPUT_GUARD                             # (an input the call does not pass: all guard)
    put = lambda name, x: arena.__setitem__(slice(regions[name][0], regions[name][0] + x.nbytes), np.ascontiguousarray(x).view(np.uint8).reshape(-1))  # noqa: E731
    put("votes", c.votes)
    put("truth", c.truth)
    if c.tokens is not None:
        put("tokens", c.tokens)
    if c.n_valid is not None:
        put("n_valid", c.n_valid)
    put("counters", c.prev)
    return arena


def pack_cells(cells):
    """include/scvote.h SCV_FLAG_PACKED_CELLS: max_count | truth_count << 7 | n_modes << 14 | min_mode << 21 | hit << 31; an empty cell has min_mode 1023."""
    mm = np.where(cells["max_count"] == 0, 1023, cells["min_mode"].astype(np.int64)).astype(np.uint32)
    return (cells["max_count"].astype(np.uint32) | (cells["truth_count"].astype(np.uint32) << 7) | (cells["n_modes"].astype(np.uint32) << 14) |
            (mm << 21) | (cells["hit"].astype(np.uint32) << 31)).astype(np.uint32)


def oracle_outputs(c):
    """What oracle.coracle says about the call (prefix budgets: the dense expansion)."""
    votes, tokens = c.votes, c.tokens
    if c.prefix:
        votes = np.ascontiguousarray(np.broadcast_to(votes[:, None, :], (c.P, c.B, c.N)))
        tokens = None if tokens is None else np.ascontiguousarray(np.broadcast_to(tokens[:, None, :], (c.P, c.B, c.N)))
    out = coracle.aggregate(votes, c.truth, tokens=tokens, n_valid=c.n_valid)
    assert out["rc"] == 0, (c.seed, out["rc"])
    return out


def expected_arena(c, regions, arena, out):
    """The arena the call must leave behind: the one it was given, with the requested outputs written -- and nothing else changed."""
    want = arena.copy()
    put = lambda name, x: want.__setitem__(slice(regions[name][0], regions[name][0] + x.nbytes), np.ascontiguousarray(x).view(np.uint8).reshape(-1))  # noqa: E731
    sums = np.concatenate([out["tie_class_hits"].reshape(-1), out["token_sum"] if c.tokens_on else np.zeros(c.B, np.int64), out["truth_count_sum"]])
    put("counters", sums if c.overwrite else c.prev + sums)
    if c.want_cells:
        put("cells", pack_cells(out["cells"]) if c.packed else out["cells"])
    if c.ctok_given and c.tokens_on:
        put("cell_tokens", out["cell_tokens"])
    return want


def check(c, regions, want, got, err_word=0):
    """One comparison of the whole arena; the message names the stratum, the table nearest to the first changed byte, the offset relative to it
    and the bytes found."""
    assert err_word == 0, f"seed {c.seed} ({c.stratum}): error word {err_word:#x}"
    assert got.shape == want.shape
    if np.array_equal(got, want):
        return
    at = int(np.flatnonzero(got != want)[0])
    name, (o, n) = min(regions.items(), key=lambda kv: 0 if kv[1][0] <= at < kv[1][0] + kv[1][1] else min(abs(at - kv[1][0]), abs(at - kv[1][0] - kv[1][1] + 1)))
    where = f"{name}{at - o:+d}" if o <= at < o + n else (f"{at - o} bytes before {name}" if at < o else f"{at - (o + n)} bytes behind the end of {name}")
    raise AssertionError(f"seed {c.seed} ({c.stratum}; P={c.P} B={c.B} N={c.N} prefix={c.prefix} tokens={c.tokens_on} cells={c.want_cells} packed={c.packed} "
                         f"overwrite={c.overwrite} ctok_given={c.ctok_given} requested={requested(c)[name] if name in OUTPUTS else 'input'} opts={c.opts}): "
                         f"first changed byte at {where}: found {got[at:at + 16].tobytes().hex()} want {want[at:at + 16].tobytes().hex()}")


# ---- which kernel a draw reaches: queries for tests/plan_check.cpp ----------------------------------------------------------------------------------

KINDS = ("LANE", "SORT", "REG", "STREAM")


def plan_queries(c):
    """Lines for plan_check's standard input; plan_of reads the answers back (8 answers per draw)."""
    ra, tok, ncells = int(rows_aligned(c)), int(c.tokens_on), c.P * c.B
    bases = int(c.align["votes"] == 0 and (not c.tokens_on or c.align["tokens"] == 0))
    opts = {k: v for k, v in c.opts.items() if k not in ("grid", "segs")}
    if "segs" in c.opts:
        opts["segs_override"] = c.opts["segs"]
    if c.prefix and c.budgets_host and c.opts.get("prefix_path", 0) == 0 and promise_ok(c):
        opts["prefix_path"] = 5
    opts["overwrite_counters"] = int(c.overwrite)
    lines = ["reset"] + [f"opt {k} {v}" for k, v in opts.items()]
    nreg = c.N if ra else c.N + 3
    lines += [f"kind {c.N} {c.B} {ra} {tok} 0", f"few {c.N} {c.B} {ncells} {bases} 0 {c.opts.get('grid', 0)}", f"shape {nreg} {c.opts.get('reg_shape', 0)} 0",
              f"split {c.N} {ncells} {256 * 8}", f"reduce 1 1 {ncells} {c.B} {c.N}", f"owfew 1 {ncells} {c.B}",
              f"spe {c.P} {c.B} {c.N} {ra}", f"plane {c.B} {c.N} {tok}"]
    return lines


def promise_ok(c):
    N = c.N
    cap = 16 if N <= 32 else (32 if N <= 64 else 64)
    return 16 < N <= 128 and N % 4 == 0 and all(n <= 0 or n >= N or ((n & (n - 1)) == 0 and n <= cap) for n in c.budgets)


def plan_of(c, answers, form_answer=None):
    """The kernel family of the draw from plan_check's eight answers (and, for a prefix draw, the answer to its `form` query)."""
    kind, few, shape, split, reduce, owfew, spe, plane = answers
    if c.prefix:
        if int(spe) and promise_ok(c):           # (not promised: the general kernel is queued behind it and leaves)
            return "scv_sort_prefix2" if c.N > 64 else "scv_sort_prefix"
        return "prefix_" + form_answer
    if kind == "LANE":
        ok, one, _ = (int(x) for x in few.split())
        return ("scv_one_vote" if c.N == 1 else "scv_two_votes") if one else ("scv_few_votes" if ok else "scv_lane_cells")
    if kind == "REG":
        g, v, h = (int(x) for x in shape.split())
        return f"reg_{1000 + 10 * v + h}" if h else f"reg_{100 * g + v}"
    if kind == "STREAM":
        S = int(split.split()[0])
        if S > 1:
            return "stream_split"
        return "stream_reduce" if (int(reduce) and not int(owfew)) else "stream"
    return "scv_sort_cells"
