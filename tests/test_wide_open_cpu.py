"""CPU tests of the open answer domain of scv_resample_wide_i32 (SCV_FLAG_OPEN_DOMAIN on pools of up to 4096 samples): the numpy mirror
(o1_inference_scaling_laws_amd/wide.py, open_domain=True) against a naive loop over collections.Counter on the raw values, the flag's
identity on pools inside 0..1023, the relabelling property, and the rule for tie classes beyond the table (n_modes >= 1025).
Also the row and pool builders that tests/test_gpu_wide_open.py shares."""
from collections import Counter

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import synth, wide
from o1_inference_scaling_laws_amd.resample import ERR_CLASS_BIT, TIE_CLASSES
from tests._open_domain import I32_MAX, I32_MIN, relabel, row_of

WIDE_CLASSES = ("equal", "distinct", "two", "edges", "hash", "d1023", "d1024", "d1025")
TRUTHS = ("absent", "smallest", "largest", "present", "modal")


def wide_row(rng, N, cls):
    """One row of N int32 votes (int64 array inside the int32 range) of a value class of the wide entry; classes of tests/_open_domain.py
    (few, special, bitpairs, mixed) pass through to row_of."""
    if cls == "equal":
        return np.full(N, int(rng.choice([I32_MIN, -7, 5, 1024, I32_MAX])), dtype=np.int64)
    if cls == "distinct":                                                  # D = N, INT32_MIN and INT32_MAX among them
        v = rng.choice(2 ** 22, size=N, replace=False).astype(np.int64) * 1021 - 2 ** 31 + 1
        v[0] = I32_MIN
        if N > 1:
            v[1] = I32_MAX
        return rng.permutation(v)
    if cls == "two":
        a, b = (int(x) for x in rng.choice([I32_MIN, -1, 0, 1023, 1024, 77777, I32_MAX], size=2, replace=False))
        v = np.where(rng.random(N) < 0.5, a, b).astype(np.int64)
        v[0] = a
        v[-1] = b if N > 1 else a
        return v
    if cls == "edges":                                                     # both ends of the range, and values around the old domain
        pal = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1023, 1024, I32_MAX - 1, I32_MAX], dtype=np.int64)
        v = pal[rng.integers(0, len(pal), N)]
        v[: min(N, len(pal))] = rng.permutation(pal)[: min(N, len(pal))]
        return rng.permutation(v)
    if cls == "hash":                                                      # 32-bit hashes with a peak
        v = rng.integers(I32_MIN, I32_MAX + 1, size=N, dtype=np.int64)
        v[rng.random(N) < 0.3] = int(v[0])
        return v
    if cls.startswith("d") and cls[1:].isdigit():                          # exactly D distinct values (D <= N), every one present
        D = int(cls[1:])
        vals = rng.choice(2 ** 22, size=D, replace=False).astype(np.int64) * 1021 - 2 ** 31 + 5
        v = np.concatenate([vals, vals[rng.integers(0, D, N - D)]])
        return rng.permutation(v)
    return row_of(rng, N, cls)


def truth_for(rng, row, kind):
    u, c = np.unique(row, return_counts=True)
    if kind == "absent":
        t = int(rng.integers(I32_MIN, I32_MAX))
        while (row == t).any():
            t = t + 1 if t < I32_MAX else I32_MIN
        return t
    if kind == "smallest":
        return int(u[0])
    if kind == "largest":
        return int(u[-1])
    if kind == "modal":
        return int(u[np.argmax(c)])
    return int(row[rng.integers(0, len(row))])


def wide_pool(rng, N, classes, truths=TRUTHS, shift=0):
    """pool int32 [len(classes), N], one row per class; truth int32, its kinds cycling through ``truths`` from ``shift``."""
    rows = [wide_row(rng, N, c) for c in classes]
    truth = [truth_for(rng, r, truths[(i + shift) % len(truths)]) for i, r in enumerate(rows)]
    return np.stack(rows).astype(np.int32), np.array(truth, dtype=np.int64).astype(np.int32)


def relabel_wide(pool, truth):
    """tests/_open_domain.py relabel for rows of up to 1024 distinct values: an absent truth becomes -1 (code 1023 may be taken here)."""
    enc, tcode = relabel(pool, truth)
    for p in range(pool.shape[0]):
        if not (pool[p] == truth[p]).any():
            tcode[p] = -1
    return enc, tcode


def naive(pool, truth, nv, r0, r1, seed, tokens=None, p_offset=0, M=None):
    """The header's text, literally: per (problem, resample, budget) a Counter over the raw values of the prefix."""
    P, N = pool.shape
    B, R = len(nv), r1 - r0
    tie = np.zeros((B, TIE_CLASSES), dtype=np.int64)
    tok = np.zeros(B, dtype=np.int64)
    tcs = np.zeros(B, dtype=np.int64)
    per = None if M is None else np.zeros((R, B, M), dtype=np.int64)
    err = 0
    for p in range(P):
        order = wide.orderings(seed, p_offset + p, np.arange(r0, r1), N)
        for ri in range(R):
            for b in range(B):
                k = int(np.clip(nv[b], 0, N))
                if k == 0:
                    continue
                idx = order[ri, :k]
                c = Counter(pool[p][idx].tolist())
                maxc = max(c.values())
                nm = sum(1 for x in c.values() if x == maxc)
                tc = c.get(int(truth[p]), 0)
                tcs[b] += tc
                if tokens is not None:
                    tok[b] += int(tokens[p][idx].astype(np.int64).sum())
                if tc != maxc:
                    continue
                if nm >= TIE_CLASSES:
                    err |= ERR_CLASS_BIT
                    continue
                tie[b, nm] += 1
                if per is not None:
                    if nm < M:
                        per[ri, b, nm] += 1
                    else:
                        err |= ERR_CLASS_BIT
    return tie, tok, tcs, per, err


def same(a, b, tokens=True):
    assert np.array_equal(a.tie_class_hits, b.tie_class_hits)
    assert np.array_equal(a.truth_count_sum, b.truth_count_sum)
    if tokens:
        assert np.array_equal(a.token_sum, b.token_sum)
    assert (a.per_resample is None) == (b.per_resample is None)
    if a.per_resample is not None:
        assert np.array_equal(a.per_resample, b.per_resample)
    assert a.error_bits == b.error_bits


@pytest.mark.parametrize("N", [1, 2, 7, 65, 300, 1100])
def test_open_mirror_against_a_naive_loop(N):
    rng = np.random.default_rng(500 + N)
    classes = ["equal", "distinct", "two", "edges", "hash", "mixed"] + (["d1023", "d1024", "d1025"] if N >= 1025 else [])
    pool, truth = wide_pool(rng, N, classes, shift=N)
    tokens = rng.integers(0, 90, size=pool.shape).astype(np.int32)
    nv = np.array([0, 1, 2, N // 2, N - 1, N, N + 4, -1], dtype=np.int32)
    M = N + 1 if N < 1000 else 700                                         # 700: the all-distinct rows overflow per_resample
    R = 3 if N < 1000 else 2
    got = wide.resample_wide(pool, truth, nv, 5, 5 + R, seed=N, tokens=tokens, p_offset=9, M=M, open_domain=True)
    tie, tok, tcs, per, err = naive(pool, truth, nv, 5, 5 + R, N, tokens, 9, M)
    assert np.array_equal(got.tie_class_hits, tie) and np.array_equal(got.token_sum, tok)
    assert np.array_equal(got.truth_count_sum, tcs) and np.array_equal(got.per_resample, per)
    assert got.error_bits == err
    assert got.tie_class_hits.shape == (len(nv), TIE_CLASSES)


@pytest.mark.parametrize("dist", range(6))
def test_in_domain_pools_are_the_same_with_the_flag_on_and_off(dist):
    N = (40, 300, 1024, 1500, 70, 513)[dist]
    a, t, tr = synth.fill(4, 1, N, 10 + dist, dist, want_tokens=True)
    pool, tok = a[:, 0, :].copy(), t[:, 0, :].copy()
    nv = np.array([1, 2, 3, N // 3, N, 0], dtype=np.int32)
    off = wide.resample_wide(pool, tr, nv, 2, 9, seed=3, tokens=tok, p_offset=4, M=N + 1)
    on = wide.resample_wide(pool, tr, nv, 2, 9, seed=3, tokens=tok, p_offset=4, M=N + 1, open_domain=True)
    assert off.error_bits == 0
    same(on, off)


@pytest.mark.parametrize("N", [3, 64, 600, 1024, 2048])
def test_relabelled_pool_with_the_flag_off_equals_the_flag_on_mirror(N):
    rng = np.random.default_rng(900 + N)
    classes = ["equal", "two", "edges", "special"] + (["hash", "distinct"] if N <= 1024 else ["d1023", "d1024"])    # D <= 1024 in every row
    pool, truth = wide_pool(rng, N, classes, shift=N)
    assert all(len(np.unique(r)) <= 1024 for r in pool)
    enc, tcode = relabel_wide(pool, truth)
    nv = np.array([1, 2, N // 2, N], dtype=np.int32)
    on = wide.resample_wide(pool, truth, nv, 0, 4, seed=N, M=N + 1, open_domain=True)
    off = wide.resample_wide(enc, tcode, nv, 0, 4, seed=N, M=N + 1)
    assert off.error_bits == 0
    same(on, off, tokens=False)


def test_a_tie_class_beyond_the_table_is_an_error_and_counted_nowhere():
    N, R = 1025, 3
    row = wide_row(np.random.default_rng(1), N, "distinct")
    pool = row[None, :].astype(np.int32)
    truth = np.array([row[17]], dtype=np.int64).astype(np.int32)
    tokens = np.full((1, N), 2, dtype=np.int32)
    nv = np.array([1024, 1025], dtype=np.int32)
    res = wide.resample_wide(pool, truth, nv, 0, R, seed=4, tokens=tokens, M=1100, open_domain=True)
    hits = int(res.tie_class_hits[0, 1024])                                # every 1024-prefix that holds the truth: a 1024-way tie, the last column
    assert res.tie_class_hits[0].sum() == hits == res.truth_count_sum[0] and 0 < hits <= R
    assert res.error_bits == ERR_CLASS_BIT                                 # budget 1025: n_modes = 1025 has no column
    assert res.tie_class_hits[1].sum() == 0 and res.per_resample[:, 1, :].sum() == 0
    assert res.truth_count_sum[1] == R and list(res.token_sum) == [R * 1024 * 2, R * 1025 * 2]
    only = wide.resample_wide(pool, truth, nv[:1], 0, R, seed=4, M=1100, open_domain=True)
    assert only.error_bits == 0 and int(only.tie_class_hits[0, 1024]) == hits
    absent = np.array([truth_for(np.random.default_rng(2), row, "absent")], dtype=np.int64).astype(np.int32)
    res = wide.resample_wide(pool, absent, nv, 0, R, seed=4, M=1100, open_domain=True)
    assert res.error_bits == 0 and res.tie_class_hits.sum() == 0 and res.truth_count_sum.sum() == 0
