"""CPU tests of the token-budget vote over wide pools (include/scvote.h scv_token_budget_wide_i32): the numpy mirror
(o1_inference_scaling_laws_amd/wide_budget.py) against a naive restatement of the header text (tests/independent_wide_budget.py), against the
mirror of scv_token_budget_prefix_i32 in pool order, against the mirror of scv_resample_wide_i32 with equal tokens, the edges of the budget
axis, and the curve records.  No GPU.  Every comparison is on integers, bit for bit."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import curves, synth, token_budget, wide, wide_budget
from o1_inference_scaling_laws_amd.engine import decode_min_mode
from tests import independent_wide_budget as ind


def pool_of(P, N, seed, dist):
    a, t, tr = synth.fill(P, 1, N, seed, dist, want_tokens=True)
    return a[:, 0, :].copy(), t[:, 0, :].copy(), tr


def same_as_naive(res, nv, pool, open_domain):
    assert np.array_equal(res.tie_class_hits, nv["tie"])
    assert np.array_equal(res.token_sum, nv["token_sum"])
    assert np.array_equal(res.vote_count_sum, nv["vote_count_sum"])
    assert np.array_equal(res.truth_count_sum, nv["truth_count_sum"])
    if nv["per"] is not None:
        assert np.array_equal(res.per_resample, nv["per"])
    assert res.error_bits == nv["err"]
    if res.cells is not None:
        assert np.array_equal(res.cell_tokens, nv["cell_tokens"])
        mm = decode_min_mode(pool, res.cells) if open_domain else res.cells["min_mode"].astype(np.int64)
        for p in range(res.cells.shape[0]):
            for b in range(res.cells.shape[1]):
                c = res.cells[p, b]
                assert (int(c["max_count"]), int(c["truth_count"]), int(c["n_modes"]), int(mm[p, b]), int(c["hit"])) == nv["cells"][p][b], (p, b)


CASES = [  # (P, N, R (None: pool order), r_begin, p_offset, dist, fold, budgets)
    (3, 1, 4, 0, 0, 1, 0, [0, -1, 10 ** 6, 700]),
    (2, 2, None, 0, 5, 0, 2, [1500, 0, 1500, -5, 1 << 40]),
    (3, 7, 6, 3, 1 << 33, 3, 0, [4000, 900, 0, 1 << 62, 2500, 2500]),
    (3, 7, None, 0, 0, 3, 3, [4000, 900, 0, 1 << 62, 2500]),
    (2, 65, 3, 2 ** 31 - 1 - 3, 0, 4, 3, [1 << 11, 1 << 13, 1 << 15, 1 << 17, -(1 << 62), 30000]),
    (2, 300, 2, 1, 2, 1, 0, [1 << 18, 1 << 12, 150000, 1 << 30, 77]),
    (2, 300, None, 0, 2, 1, 7, [1 << 18, 1 << 12, 150000, 1 << 30, 77]),
]


@pytest.mark.parametrize("open_domain", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_mirror_equals_the_naive_restatement(case, open_domain):
    P, N, R, r0, p_off, dist, fold, budgets = CASES[case]
    pool, tok, tr = pool_of(P, N, 170 + case, dist)
    if fold:
        pool, tr = pool % fold, (tr % fold).astype(np.int32)
    if open_domain:                                                      # values over the whole int32 range, equality preserved
        pool = (pool.astype(np.int64) * 2654435761 % (1 << 32) - (1 << 31)).astype(np.int32)
        tr = (tr.astype(np.int64) * 2654435761 % (1 << 32) - (1 << 31)).astype(np.int32)
    elif case % 2:
        tr[0] = (1023, -3, 2000)[case % 3]
        pool[0, 0] = 5000                                                # error bit 0, bin 1023
    r1 = None if R is None else r0 + R
    M = N + 1
    res = wide_budget.token_budget_wide(pool, tok, tr, budgets, r0, r1, seed=900 + case, p_offset=p_off, M=M, want_cells=R is None,
                                        open_domain=open_domain)
    nv = ind.naive_wide_budget(pool.tolist(), tok.tolist(), tr.tolist(), budgets, r0, r1, 900 + case, p_off, M, open_domain)
    same_as_naive(res, nv, pool, open_domain)


@pytest.mark.parametrize("open_domain", [False, True])
@pytest.mark.parametrize("N", [1, 5, 64, 200, 256])
def test_pool_order_equals_the_prefix_mirror_in_every_field(N, open_domain):
    pool, tok, tr = pool_of(4, N, 31 + N, 1 if N % 2 else 3)
    if open_domain:
        pool = (pool.astype(np.int64) * 40503 - 7000).astype(np.int32)
        tr = (tr.astype(np.int64) * 40503 - 7000).astype(np.int32)
    total = int(tok.sum(axis=1).max())
    budgets = [total, 0, -1, total // 3, total // 3, int(tok[0, 0]), int(tok[0, 0]) - 1, total + 1, total // 50]
    a = wide_budget.token_budget_wide(pool, tok, tr, budgets, M=N + 1, want_cells=True, open_domain=open_domain)
    b = token_budget.token_budget_prefix(pool, tok, tr, budgets, M=N + 1, want_cells=True, open_domain=open_domain)
    for f in ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum", "per_resample", "cell_tokens"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.cells.tobytes() == b.cells.tobytes()
    assert a.error_bits == b.error_bits and (a.P, a.R) == (b.P, b.R)


@pytest.mark.parametrize("N,c", [(300, 1), (300, 977), (1024, 40)])
def test_equal_tokens_reduce_to_the_sample_budgets_of_resample_wide(N, c):
    P, R = 3, 4
    pool, _, tr = pool_of(P, N, 5 + N, 1)
    tok = np.full((P, N), c, dtype=np.int32)
    ks = np.array([1, 2, N // 3, N - 1, N, 17, 17, 0], dtype=np.int64)
    budgets = c * ks + (c - 1)
    a = wide_budget.token_budget_wide(pool, tok, tr, budgets, 2, 2 + R, seed=77, p_offset=3)
    w = wide.resample_wide(pool, tr, ks, 2, 2 + R, seed=77, tokens=tok, p_offset=3)
    assert np.array_equal(a.tie_class_hits, w.tie_class_hits)
    assert np.array_equal(a.truth_count_sum, w.truth_count_sum)
    assert np.array_equal(a.token_sum, w.token_sum)
    assert np.array_equal(a.vote_count_sum, P * R * ks)


def test_budget_edges():
    P, N = 2, 40
    pool, tok, tr = pool_of(P, N, 9, 1)
    # negative, zero and 2^62 budgets
    res = wide_budget.token_budget_wide(pool, tok, tr, [-1, -(1 << 62), 0, 1 << 62], 0, 3, seed=1)
    assert res.vote_count_sum.tolist() == [0, 0, 0, P * 3 * N] and res.tie_class_hits[:3].sum() == 0 and res.token_sum[3] == 3 * int(tok.sum())
    # all-zero tokens: every budget >= 0 takes the whole pool
    z = wide_budget.token_budget_wide(pool, np.zeros_like(tok), tr, [-1, 0, 5], 0, 2, seed=1)
    assert z.vote_count_sum.tolist() == [0, P * 2 * N, P * 2 * N] and z.token_sum.tolist() == [0, 0, 0]
    assert np.array_equal(z.tie_class_hits[1], z.tie_class_hits[2]) and z.tie_class_hits[1].sum() > 0
    # a budget exactly equal to a running sum fits; one token less does not
    run = np.cumsum(tok[0].astype(np.int64))
    e = wide_budget.token_budget_wide(pool[:1], tok[:1], tr[:1], [int(run[6]), int(run[6]) - 1], want_cells=True)
    assert e.vote_count_sum.tolist() == [7, 6] and e.cell_tokens[0].tolist() == [int(run[6]), int(run[5])]
    # a zero-token sample behind the last one that fits is still taken
    t2 = tok[:1].copy()
    t2[0, 7] = 0
    e = wide_budget.token_budget_wide(pool[:1], t2, tr[:1], [int(run[6])], want_cells=True)
    assert e.vote_count_sum.tolist() == [8]
    # a negative token count: error bit 4
    t2[0, 3] = -5
    assert wide_budget.token_budget_wide(pool[:1], t2, tr[:1], [100]).error_bits & token_budget.ERR_TOKEN_BIT


def test_largest_tokens_at_the_largest_pool_do_not_overflow():
    N = 4096
    pool = (np.arange(N, dtype=np.int32) % 3).reshape(1, N)
    tok = np.full((1, N), 2 ** 31 - 1, dtype=np.int32)
    tr = np.array([0], dtype=np.int32)
    full = N * (2 ** 31 - 1)
    assert full < 2 ** 43
    res = wide_budget.token_budget_wide(pool, tok, tr, [full, full - 1, 1 << 62, 2 ** 31 - 2], 0, 2, seed=3)
    assert res.vote_count_sum.tolist() == [2 * N, 2 * (N - 1), 2 * N, 0]
    assert res.token_sum.tolist() == [2 * full, 2 * (full - (2 ** 31 - 1)), 2 * full, 0]
    p = wide_budget.token_budget_wide(pool, tok, tr, [full, (2 ** 31 - 1) * 5], want_cells=True)
    assert p.cell_tokens[0].tolist() == [full, (2 ** 31 - 1) * 5] and p.cells["max_count"][0].tolist() == [1366, 2]


def test_more_than_1024_tied_values_have_no_column():
    N = 2100
    pool = np.arange(N, dtype=np.int32).reshape(1, N) * 1000 - 10 ** 6       # all distinct: every prefix ties n ways
    tok = np.ones((1, N), dtype=np.int32)
    tr = pool[:, 0].copy()
    res = wide_budget.token_budget_wide(pool, tok, tr, [1024, 1025, 5], want_cells=True, open_domain=True, M=1025)
    assert res.error_bits == 2                                            # the 1025-way tie: counted in neither table, its sums still added
    assert res.tie_class_hits[0, 1024] == 1 and res.tie_class_hits[1].sum() == 0 and res.tie_class_hits[2, 5] == 1
    assert res.per_resample[0, 1].sum() == 0 and res.vote_count_sum.tolist() == [1024, 1025, 5] and res.truth_count_sum.tolist() == [1, 1, 1]
    assert res.cells["n_modes"][0].tolist() == [1024, 1025, 5] and res.cells["hit"][0].tolist() == [1, 1, 1]


def test_slices_of_r_and_shards_of_p_add_up():
    P, N, R = 4, 90, 6
    pool, tok, tr = pool_of(P, N, 12, 3)
    budgets = [1 << 12, 1 << 14, 1 << 16, 0]
    whole = wide_budget.token_budget_wide(pool, tok, tr, budgets, 0, R, seed=4, M=N + 1)
    parts = [wide_budget.token_budget_wide(pool[p0:p1], tok[p0:p1], tr[p0:p1], budgets, r0, r1, seed=4, p_offset=p0, M=N + 1)
             for (p0, p1) in ((0, 1), (1, 4)) for (r0, r1) in ((0, 2), (2, 6))]
    for f in ("tie_class_hits", "token_sum", "vote_count_sum", "truth_count_sum"):
        assert np.array_equal(getattr(whole, f), sum(getattr(x, f) for x in parts)), f
    assert np.array_equal(whole.per_resample[:2], parts[0].per_resample + parts[2].per_resample)


def test_curve_records_follow_the_mirror():
    P, N, R = 3, 300, 3
    pool, tok, tr = pool_of(P, N, 2, 1)
    budgets = [1 << 12, 1 << 15, 1 << 20]

    class MirrorEngine:
        def token_budget_wide(self, pool, tokens, truth, token_budgets, resamples=None, seed=0, **kw):
            return wide_budget.token_budget_wide(pool, tokens, truth, token_budgets, 0, resamples, seed)

    recs = curves.wide_token_budget_records(MirrorEngine(), pool, tr, tok, budgets, resamples=R, seed=8)
    ref = wide_budget.token_budget_wide(pool, tok, tr, budgets, 0, R, seed=8)
    assert [r["token_limit"] for r in recs] == budgets
    for b, r in enumerate(recs):
        assert r["accuracy"] == ref.accuracy(b) and r["avg_tokens_used"] == float(ref.avg_tokens_used(b)) and r["avg_votes"] == float(ref.avg_votes(b))


def test_the_bench_tool_restates_the_launch_shape_of_the_header(tmp_path):
    """The wide bench tools print lanes and LDS bytes per launch from ONE restatement of csrc/scvote_dispatch.h (tools/wide_bench.py, which
    wide_open_bench.py and wide_budget_bench.py import): a host-only program that includes the header prints the real ones (no GPU, no
    device code)."""
    import importlib.util
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(repo, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    geo, tool, open_tool = load("wide_bench"), load("wide_budget_bench"), load("wide_open_bench")
    src = tmp_path / "shape.cpp"
    hdr = os.path.join(repo, "o1_inference_scaling_laws_amd", "csrc", "scvote_dispatch.h")
    src.write_text('#include "%s"\n#include <cstdio>\nint main() {\n'
                   '    for (int N : {1, 2, 3, 64, 65, 128, 129, 300, 512, 513, 1000, 1024, 1025, 2048, 4095, 4096}) for (int B : {1, 12, 13, 32}) for (int o = 0; o < 2; ++o)\n'
                   '        printf("%%d %%d %%d %%d %%lld %%lld\\n", N, B, o, scv::wide_lanes(N), 4 * scv::wide_budget_lds_words(N, B, o != 0),\n'
                   '               4 * scv::wide_lds_words(N, B, o != 0));\n}\n' % hdr)
    exe = tmp_path / "shape"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O0", "-o", str(exe), str(src)],
                   check=True, stderr=subprocess.DEVNULL, timeout=300)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    rows = [tuple(int(x) for x in r.split()) for r in rows if r]
    assert len(rows) == 16 * 4 * 2
    for N, B, o, lanes, lds, wide_lds in rows:
        assert (geo.wide_lanes(N), 4 * geo.wide_budget_lds_words(N, B, bool(o)), 4 * geo.wide_lds_words(N, B, bool(o))) == (lanes, lds, wide_lds), (N, B, o)
        assert tool.launch_shape(N, B, bool(o))[:2] == (lanes, lds), (N, B, o)
        assert open_tool.launch_shape(N, B, bool(o))[:2] == (lanes, wide_lds), (N, B, o)
        if not o:
            assert geo.launch_shape(N, B)[:2] == (lanes, wide_lds), (N, B)
