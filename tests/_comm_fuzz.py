"""Seeded draws for the one-process communicator (csrc/scvote_comm.hip: scv_allreduce_counters, scv_allgather_i64, scv_allgather_cells):
``draw(seed)`` returns one SEQUENCE for one communicator -- a rank count, every rank's int64 backing array (guard words on both sides of a
working buffer that starts at word 3 or 4 of it) and 6 .. 12 ops, collectives back to back on that one buffer with torch writes and stream
changes between them -- that depends on the seed alone; ``model(sequence)`` is what every rank's backing array must hold afterwards, in plain
numpy.  No GPU, no torch: tests/test_comm_fuzz_cpu.py checks the model against a word-by-word statement, what the draws reach and that they tell
wrong collectives from the right ones; tests/test_gpu_comm_fuzz.py holds the C ABI and ``MultiDeviceEngine`` to them.

An op is a tuple:
    ("allreduce", count)             words [0, count) of every rank's working buffer <- their sum over the ranks (int64, wrapping)
    ("allgather_i64", counts[G])     rank j's block of counts[j] words sits at word sum(counts[:j]); afterwards every rank has every block
    ("allgather_cells", rows[G], B)  the same over 16-byte cells: rank j's block is rows[j] * B cells = 2 * rows[j] * B words
    ("write", rank, a, b)            buf.mul_(a).add_(b) over that rank's WHOLE working buffer (int64, wrapping): device work between two
                                     collectives that rewrites their buffer, enqueued without a host sync
    ("rebind",)                      the next collective is issued under another torch stream (the Python layer only; the C ABI skips it)

The draws are stratified over the seed so that few seeds reach every edge: the rank count is G_CHOICES[(seed // 12) % 5] and the first
all-reduce of a draw takes AR_EDGES[(seed + seed // 12) % 12] -- 60 consecutive seeds hold every (rank count, edge) pair once.

Work bound of one sequence: the sum over its ops of (words moved * G; a write: the working buffer once) <= WORK // work_div."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

STREAM = 8_300_000                                                       # default_rng((STREAM, seed))
DEFAULT_SEEDS = 60                                                       # what tests/test_gpu_comm_fuzz.py runs and tests/test_comm_fuzz_cpu.py proves reach on
WORK = 4_000_000
GUARD = 3                                                                # guard words behind the working buffer; 3 or 4 before it
G_CHOICES = (1, 2, 3, 5, 8)
GRID_STRIDE_WORDS = 64 * 256                                             # scv_sum_peers_k: at most 64 workgroups of 256 lanes -- above this the loop strides
STAGING_WORDS = (1 << 20) // 8                                           # the staging buffer of a new communicator (kTmpBytesAtCreate)
AR_EDGES = (0, 1, 255, 256, 257, 8217, 16383, 16384, 16385, 131071, 131072, 131073)
AR_RANDOM_MAX = 300_000
CELL_B = (1, 3, 8, 32)
VALUE_KINDS = ("small", "full", "minus1", "one_rank")
GATHER_KINDS = ("ragged", "all_zero", "one_owner", "ones")
OP_KINDS = ("allreduce", "allgather_i64", "allgather_cells", "write", "rebind")
OP_P = (0.34, 0.18, 0.14, 0.24, 0.10)
MASK = (1 << 64) - 1


def _i64(rng, n):
    return rng.integers(-2 ** 63, 2 ** 63, size=n, dtype=np.int64)


def _gather_counts(rng, G, cap_total, unit):
    """Block sizes of one all-gather in units of ``unit`` words (1: int64 words; 2 * B: rows of B cells), sum * unit <= cap_total."""
    kind = str(rng.choice(GATHER_KINDS, p=[0.55, 0.10, 0.20, 0.15]))
    cap = max(cap_total // unit, 0)
    if kind == "all_zero" or cap == 0:
        return [0] * G, "all_zero"
    if kind == "ones":
        return ([1] * G, kind) if G <= cap else ([0] * G, "all_zero")
    top = int(math.exp(rng.uniform(0.0, math.log(max(cap, 2)))))         # the largest block: log-uniform up to the whole budget
    if rng.random() < 0.25 and cap * unit > STAGING_WORDS:               # a block that crosses 1 MiB
        top = int(rng.integers(STAGING_WORDS // unit + 1, cap + 1))
    if kind == "one_owner":
        c = [0] * G
        c[int(rng.integers(0, G))] = max(top, 1)
        return c, kind
    c = [0 if rng.random() < 0.25 else int(rng.integers(1, top + 1)) for _ in range(G)]
    if G >= 2 and rng.random() < 0.6:                                    # an empty block in the first, a middle or the last rank
        c[(0, G // 2, G - 1)[int(rng.integers(0, 3))]] = 0
    while sum(c) > cap:
        c = [x // 2 for x in c]
    return c, kind


def extent(op) -> int:
    """Words of the working buffer that a collective covers."""
    if op[0] == "allreduce":
        return int(op[1])
    if op[0] == "allgather_i64":
        return int(sum(op[1]))
    if op[0] == "allgather_cells":
        return int(sum(op[1])) * int(op[2]) * 2
    return 0


def draw(seed: int, work_div: int = 1):
    """One sequence, deterministic in (seed, work_div)."""
    rng = np.random.default_rng((STREAM, int(seed)))
    q = SimpleNamespace(seed=int(seed))
    q.G = G = G_CHOICES[(seed // 12) % len(G_CHOICES)]
    q.off = int(rng.integers(3, 5))
    budget = WORK // work_div
    left = budget * 4 // 5                                               # the collectives; the writes get what is left
    n_ops = int(rng.integers(6, 13))
    ops, kinds, crossings, first_ar = [], [], 0, True
    for _ in range(n_ops):
        kind = str(rng.choice(OP_KINDS, p=OP_P))
        cap = left // G                                                  # words this op may cover
        if kind == "allreduce":
            if first_ar:
                count = AR_EDGES[(seed + seed // 12) % len(AR_EDGES)]
            elif rng.random() < 0.6:
                count = int(rng.choice(AR_EDGES))
            elif rng.random() < 0.5:
                count = int(rng.integers(0, AR_RANDOM_MAX + 1))
            else:
                count = int(math.exp(rng.uniform(0.0, math.log(AR_RANDOM_MAX))))
            if count > STAGING_WORDS and crossings == 2:                 # at most two calls above the first staging buffer: the growth and one behind it
                count = int(rng.choice([e for e in AR_EDGES if e <= STAGING_WORDS]))
            if count > cap:
                count = max([e for e in AR_EDGES if e <= cap])
            first_ar = False
            crossings += count > STAGING_WORDS
            op = ("allreduce", count)
        elif kind == "allgather_i64":
            c, gk = _gather_counts(rng, G, min(cap, AR_RANDOM_MAX), 1)
            kinds.append(gk)
            op = ("allgather_i64", tuple(c))
        elif kind == "allgather_cells":
            B = int(rng.choice(CELL_B))
            c, gk = _gather_counts(rng, G, min(cap, AR_RANDOM_MAX), 2 * B)
            kinds.append(gk)
            op = ("allgather_cells", tuple(c), B)
        elif kind == "write":
            a = int(rng.choice([1, 2, 3, -1])) if rng.random() < 0.5 else int(_i64(rng, 1)[0]) | 1
            b = int(rng.integers(0, 1000)) if rng.random() < 0.5 else int(_i64(rng, 1)[0])
            if (a, b) == (1, 0):
                b = 1
            op = ("write", int(rng.integers(0, G)), a, b)
        else:
            op = ("rebind",)
        left -= extent(op) * G
        ops.append(op)
    q.W = W = max([extent(op) for op in ops] + [1]) + int(rng.integers(0, 6))      # a few words past the largest op: never touched by a collective
    spent = sum(extent(op) * G for op in ops)
    writes = [i for i, op in enumerate(ops) if op[0] == "write"]
    while writes and spent + len(writes) * W > budget:                   # the last writes go when the buffer is too large for all of them
        ops.pop(writes.pop())
    q.ops = ops
    q.gather_kinds = tuple(kinds)
    q.work = spent + len(writes) * W
    # every rank's backing array: random guards around the working buffer
    q.value_kind = vk = str(rng.choice(VALUE_KINDS, p=[0.3, 0.4, 0.1, 0.2]))
    owner = int(rng.integers(0, G))
    q.init = []
    for r in range(G):
        back = _i64(rng, q.off + W + GUARD)
        buf = back[q.off:q.off + W]
        if vk == "small":
            buf[:] = rng.integers(0, 1000, size=W)
        elif vk == "minus1":
            buf[:] = -1
        elif vk == "one_rank" and r != owner:
            buf[:] = 0
        back.setflags(write=False)
        q.init.append(back)
    return q


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def apply(q, bufs, op, variant: str = ""):
    """One op on the ranks' working buffers (uint64 views: the arithmetic wraps).  ``variant``: one of the wrong collectives of
    tests/test_comm_fuzz_cpu.py."""
    G = q.G
    if op[0] == "allreduce":
        n = stop = op[1]
        if variant == "stops_at_16384":
            stop = min(n, GRID_STRIDE_WORDS)
        elif variant == "whole_blocks_only":
            stop = n - n % 256
        ranks = bufs[:-1] if (variant == "last_rank_left_out" and G > 1) else bufs
        total = np.sum(np.stack([b[:stop] for b in ranks]), axis=0, dtype=np.uint64)
        for r in range(G if variant != "rank0_only" else 1):
            bufs[r][:stop] = total
    elif op[0] in ("allgather_i64", "allgather_cells"):
        unit = 1 if op[0] == "allgather_i64" else 2 * op[2]
        counts = [c * unit for c in op[1]]
        off = _offsets(counts)
        for r in range(G if variant != "rank0_only" else 1):
            for j in range(G):
                if j == r:
                    continue
                dst = j * max(counts) if variant == "block_at_rank_times_max" else off[j]
                n = max(0, min(counts[j], q.W - dst))
                bufs[r][dst:dst + n] = bufs[j][off[j]:off[j] + n]
    elif op[0] == "write":
        if variant != "write_ignored":
            b = bufs[op[1]]
            b *= np.uint64(op[2] & MASK)
            b += np.uint64(op[3] & MASK)


def model(q, variant: str = ""):
    """Every rank's final backing array (int64, guards included) after the whole sequence."""
    backs = [np.array(x, dtype=np.int64) for x in q.init]
    bufs = [b[q.off:q.off + q.W].view(np.uint64) for b in backs]
    for op in q.ops:
        apply(q, bufs, op, variant)
    return backs


def describe(q) -> str:
    def short(op):
        return op[0] + "(" + ",".join(str(x).replace(" ", "") for x in op[1:]) + ")"
    return f"seed={q.seed} G={q.G} off={q.off} W={q.W} values={q.value_kind} work={q.work} ops=" + " ".join(short(op) for op in q.ops)
