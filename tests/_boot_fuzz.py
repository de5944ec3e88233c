"""Seeded draws for the problem-level bootstrap (scv_bootstrap; the same loop runs behind the grid barrier of scv_aggregate_bootstrap_i32):
``draw(seed)`` returns one complete, VALID call -- a hand-built CELL_DTYPE table [P, B], the resample range, a 64-bit seed, the class bound M,
the mode and the "boot_path" option -- that depends on the seed alone.  The bootstrap reads only ``hit`` and ``n_modes`` of a cell, so no vote
kernel runs to make a case.  No GPU, no torch: tests/test_boot_fuzz_cpu.py checks what the draws reach and that they tell wrong bootstraps
from the right one, tests/test_gpu_boot_fuzz.py holds the three device implementations to them.

The draws couple what the hand-picked shapes never did: P, B and M move the LDS fit that switches kernels (``fit_bytes``, restated from
scv_bootstrap in csrc/scvote.hip) and the B * M = 16384 counter limit; R moves against the number of workgroups of the grid-stride loop;
r_begin moves r * P across 2^32 and r_end up to 2^31 - 1; the unread fields of a cell hold random bytes.

A cell with hit = 1 has n_modes >= 1 in every table (a hit is one of the modes); misses carry any n_modes, 0 included.

Work bounds of one call: P * B * R <= WORK // work_div, and R * B * M <= OUT_WORDS (the int64 table: 32 MiB)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from oracle.coracle import CELL_DTYPE

STREAM = 8_200_000                                                       # default_rng((STREAM, seed))
DEFAULT_SEEDS = 150                                                      # what tests/test_gpu_boot_fuzz.py runs and tests/test_boot_fuzz_cpu.py proves reach on
WORK = 2_000_000
OUT_WORDS = 1 << 22
LDS_FIT_BYTES = 144 * 1024                                               # scv_bootstrap: the code table + counters of the LDS kernel
BM_MAX = 16384                                                           # B * M counters: 64 KiB of LDS
R_TOP = 2 ** 31 - 1                                                      # the largest r_end
REG_N_MAX = 8192                                                         # the default of option "reg_n_max"

P_EDGES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4097)
P_RANDOM_MAX = 75_000
B_EDGES = (1, 2, 3, 8, 16, 32)
R_EDGES = (0, 1, 2, 255, 256, 257, 511, 513)
R_RANDOM_MAX = 600
MMAX = (1, 2, 3, 7, 1024)
BM_PAIRS = ((16, 1024), (32, 512), (1, 16384))
TOP_D = (0, 1, 255, 256, 1000)
M_KINDS = ("1", "2", "3", "mmax", "mmax+1", "1025", "pair")
M_KIND_P = (0.12, 0.12, 0.10, 0.06, 0.30, 0.12, 0.18)


def fit_bytes(P: int, B: int, M: int) -> int:
    """Dynamic LDS of scv_bootstrap_lds_k: B * M counters (rounded to 4 words) + one 2-byte code per cell (rounded to 8 cells)."""
    return ((B * M + 3) & ~3) * 4 + ((P * B + 7) & ~7) * 2


def lds_kernel(c) -> bool:
    """True where scv_bootstrap runs scv_bootstrap_lds_k, False where it runs the gather kernel scv_bootstrap_k."""
    return c.boot_path != 3 and fit_bytes(c.P, c.B, c.M) <= LDS_FIT_BYTES


def _cells_at_the_fit(B: int, M: int) -> int:
    """The cell count (a multiple of 8) at which fit_bytes is exactly LDS_FIT_BYTES."""
    return (LDS_FIT_BYTES - ((B * M + 3) & ~3) * 4) // 2


def _table(rng, P, B, M, mmax, overflow):
    """CELL_DTYPE [P, B]: random bytes everywhere, then hit and n_modes.  Returns (cells, kind of table)."""
    cells = np.ascontiguousarray(rng.integers(0, 256, size=(P, B, 16), dtype=np.uint8)).view(CELL_DTYPE).reshape(P, B)
    top = min(mmax, M - 1)                                               # the largest class a hit may have in a clean table
    kind = str(rng.choice(["all_miss", "all_class1", "mixed"], p=[0.08, 0.08, 0.84]))
    if top < 1:
        kind = "all_miss"                                                # M = 1 holds no hit at all
    # misses: any n_modes (0: a cell without votes; classes at and above M: they must not matter)
    cells["n_modes"] = np.where(rng.random((P, B)) < 0.7, 1, rng.integers(0, max(mmax, 2) + 2, size=(P, B)))
    cells["hit"] = 0
    if kind == "all_class1":
        cells["hit"], cells["n_modes"] = 1, 1
    elif kind == "mixed":
        hit = rng.random((P, B)) < rng.random()
        n = np.where(rng.random((P, B)) < 0.7, 1, rng.integers(1, top + 1, size=(P, B)))
        for _ in range(3):                                               # the bound is tight: class `top` is among the hits
            p, b = int(rng.integers(0, P)), int(rng.integers(0, B))
            hit[p, b], n[p, b] = True, top
        cells["n_modes"] = np.where(hit, n, cells["n_modes"])
        cells["hit"] = hit
    if overflow:                                                         # many rows with a hit of a class >= M, so that a resample draws one
        rows = np.flatnonzero(rng.random(P) < 0.3)
        rows = np.union1d(rows, [int(rng.integers(0, P))])
        cols = rng.integers(0, B, size=rows.size)
        cells["hit"][rows, cols] = 1
        cells["n_modes"][rows, cols] = np.minimum(M + rng.integers(0, 3, size=rows.size), 65535)
    return cells, kind


def draw(seed: int, work_div: int = 1, clean: bool = False):
    """One valid call of scv_bootstrap, deterministic in (seed, work_div, clean).  ``clean``: never an overflow draw."""
    rng = np.random.default_rng((STREAM, int(seed)))
    c = SimpleNamespace(seed=int(seed))
    c.device = bool(rng.random() < 0.5)
    c.boot_path = 3 if rng.random() < 0.25 else 0
    # B, M and the largest class of the table
    B = int(rng.choice(B_EDGES))
    m_kind = str(rng.choice(M_KINDS, p=M_KIND_P))
    if m_kind == "mmax" and clean:
        m_kind = "mmax+1"
    if m_kind == "pair":
        B, M = (int(x) for x in BM_PAIRS[int(rng.integers(0, len(BM_PAIRS)))])
    m_cap = BM_MAX // B
    mmax = int(rng.choice([m for m in MMAX if m + 1 <= m_cap]))
    if m_kind in ("1", "2", "3"):
        M = int(m_kind)
    elif m_kind == "mmax":
        M = mmax                                                         # one too small: the table's largest class does not fit
    elif m_kind == "mmax+1":
        M = mmax + 1
    elif m_kind == "1025":
        M = min(1025, m_cap)
    overflow = m_kind == "mmax" or bool(rng.random() < (0.5 if M == 1 else 0.03))
    overflow = overflow and not clean
    c.B, c.M, c.m_kind, c.mmax, c.overflow = B, M, m_kind, mmax, overflow
    # P: an edge, a value at the LDS fit, or random
    p_kind = str(rng.choice(["edge", "fit", "random"], p=[0.35, 0.15, 0.50]))
    c.fit_kind = ""
    if p_kind == "edge":
        P = int(rng.choice(P_EDGES))
    elif p_kind == "fit":
        c.fit_kind = str(rng.choice(["on", "below8", "above"]))
        if c.fit_kind == "below8" and B > 8:                             # (C - 8 cells is a whole number of rows for B <= 8 only)
            c.fit_kind = "on"
        C = _cells_at_the_fit(B, M)
        P = {"on": C // B, "below8": (C - 8) // B, "above": C // B + 1}[c.fit_kind]
        if c.fit_kind == "above":
            c.boot_path = 0                                              # the gather kernel although the option asks for nothing
    else:
        P = int(rng.integers(1, P_RANDOM_MAX + 1)) if rng.random() < 0.5 else int(math.exp(rng.uniform(0.0, math.log(P_RANDOM_MAX))))
        P = max(1, min(P, WORK // work_div // (2 * B)))
    c.P, c.p_kind = P, p_kind
    # R, within the work bounds
    R = int(rng.choice(R_EDGES)) if rng.random() < 0.5 else int(rng.integers(0, R_RANDOM_MAX + 1))
    R = min(R, WORK // work_div // (P * B), OUT_WORDS // (B * M))
    # r_begin
    r_kind = str(rng.choice(["small", "2^16", "2^32/P", "top", "random"], p=[0.30, 0.18, 0.20, 1 / 6, 0.32 - 1 / 6]))
    if r_kind == "small":
        r0 = 0 if rng.random() < 0.5 else int(rng.integers(1, 8))
    elif r_kind == "2^16":
        r0 = 65536 + int(rng.integers(-300, 301))
    elif r_kind == "2^32/P":
        r0 = 2 ** 32 // P - int(rng.integers(0, R + 1))                 # r * P crosses 2^32 inside the range
    elif r_kind == "top":
        r0 = R_TOP - R - int(rng.choice(TOP_D))
    else:
        r0 = int(rng.integers(0, R_TOP - R + 1))
    c.r_kind = r_kind
    c.r_begin = max(0, min(r0, R_TOP - R))
    c.R, c.r_end = R, c.r_begin + R
    c.seed64 = (0, 2 ** 64 - 1, int(rng.integers(0, 2 ** 64, dtype=np.uint64)))[int(rng.integers(0, 3))]
    c.cells, c.table_kind = _table(rng, P, B, M, mmax, overflow)
    c.work = P * B * R
    return c


def with_range(c, r_begin: int, r_end: int):
    """The same call over another resample range (the table does not depend on the range)."""
    d = SimpleNamespace(**vars(c))
    d.r_begin, d.r_end, d.R, d.work = int(r_begin), int(r_end), int(r_end - r_begin), c.P * c.B * int(r_end - r_begin)
    return d


def find(pred, count: int, first: int = 0, limit: int = 4000, **kw):
    """The first ``count`` draws from seed ``first`` on that satisfy ``pred``."""
    out = []
    for s in range(first, first + limit):
        c = draw(s, **kw)
        if pred(c):
            out.append(c)
            if len(out) == count:
                return out
    raise LookupError(f"only {len(out)} of {count} draws found in {limit} seeds")


def cu_cases(cus: int, per_count: int = 2):
    """Clean draws whose resample count is set to CUs - 1, CUs, CUs + 1 and 2 CUs + 1 -- the tail of the grid-stride loop of
    scv_bootstrap_lds_k, whose grid is min(CUs, R) --, ``per_count`` tables each, kept inside the work bounds; r_end of the first is 2^31 - 1."""
    out = []
    for k, R in enumerate((cus - 1, cus, cus + 1, 2 * cus + 1)):
        fits = lambda c, R=R: (not c.overflow and c.boot_path == 0 and c.P >= 64 and c.P * c.B * R <= WORK and R * c.B * c.M <= OUT_WORDS
                               and fit_bytes(c.P, c.B, c.M) <= LDS_FIT_BYTES)                      # noqa: E731
        for i, c in enumerate(find(fits, per_count, first=1000 * (k + 1))):
            r0 = R_TOP - R if i == 0 else c.r_begin % (R_TOP - R)
            out.append(with_range(c, r0, r0 + R))
    return out


def draw_fused(seed: int):
    """One call of scv_aggregate_bootstrap_i32 over synthetic votes: 4097 <= N <= 6000, P * B <= 600, dist D1 / D3 / D5; odd seeds force two
    launches (boot_path = 2).  Only the streaming vote kernel can take the bootstrap into its launch, and the default dispatch gives cells of up
    to 8192 votes to the register-resident kernels: one seed in four (the even ones of them: half of the unforced calls) lowers the option
    "reg_n_max" to 4096, which hands these cells to the streaming kernel.  M comes from the cells."""
    rng = np.random.default_rng((STREAM + 1, int(seed)))
    c = SimpleNamespace(seed=int(seed))
    c.N = int(rng.choice([4097, 4100, 6000])) if rng.random() < 0.4 else int(rng.integers(4097, 6001))
    c.B = int(rng.choice([1, 2, 3, 8]))
    c.P = int(rng.integers(1, 600 // c.B + 1))
    c.dist = int(rng.choice([1, 3, 5]))
    c.synth_seed = 41_000 + int(seed)
    c.boot_path = 2 if seed & 1 else 0
    c.reg_n_max = 4096 if seed % 4 == 0 else REG_N_MAX
    c.R = R = int(rng.choice([1, 2, 255, 257, 513])) if rng.random() < 0.5 else int(rng.integers(1, R_RANDOM_MAX + 1))
    kinds = ("top", "small", "2^32/P", "2^16")
    kind = str(rng.choice(kinds))
    d = int(rng.choice(TOP_D[:2]))
    if seed % 4 == 0:                                                    # the streaming seeds take the four kinds in turn, "top" ending at 2^31 - 1
        kind, d = kinds[(seed // 4) % 4], 0
    r0 = {"small": int(rng.integers(0, 8)), "2^16": 65536 - R // 2, "2^32/P": 2 ** 32 // c.P - R // 2, "top": R_TOP - R - d}[kind]
    c.r_begin = max(0, min(r0, R_TOP - R))
    c.r_end = c.r_begin + R
    c.r_kind = kind
    c.seed64 = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    c.extra_classes = int(rng.choice([0, 0, 1, 1000]))                   # M = largest class of a hit + 1 + extra
    return c


def describe(c) -> str:
    keys = ("seed", "P", "B", "M", "R", "r_begin", "r_end", "seed64", "device", "boot_path", "m_kind", "mmax", "p_kind", "fit_kind", "r_kind",
            "table_kind", "overflow", "N", "dist", "reg_n_max")
    return " ".join(f"{k}={getattr(c, k)}" for k in keys if hasattr(c, k))
