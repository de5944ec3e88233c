"""Randomised parity of the three device implementations of the problem-level bootstrap -- scv_bootstrap_k (global gathers), scv_bootstrap_lds_k
(code table in LDS, grid-stride over the resamples) and the same loop behind the grid barrier of the vote kernel (scv_aggregate_bootstrap_i32)
-- against the C oracle, whole tables, bit for bit: 150 seeded calls of tests/_boot_fuzz.py in both modes (what they reach and that they
discriminate: tests/test_boot_fuzz_cpu.py), resample counts around the CU count, both kernels on one draw, slices that concatenate, the
vote + bootstrap call in both of its forms, who owns the error word between a DEVICE call and a HOST bootstrap, 20 sequences of 10 mixed calls
on one context, and the refusals.  Ranges up to r_end = 2^31 - 1 are part of every group.

SCV_FUZZ_BOOT_SEEDS / SCV_FUZZ_BOOT_MIXED and SCV_FUZZ_FIRST move the seed ranges."""
import os

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib, synth
from oracle import coracle
from tests import _boot_fuzz as bf
from tests import _vote_fuzz as vf

pytestmark = pytest.mark.gpu

FIRST = int(os.environ.get("SCV_FUZZ_FIRST", "0"))
BOOT_SEEDS = int(os.environ.get("SCV_FUZZ_BOOT_SEEDS", str(bf.DEFAULT_SEEDS)))
MIXED_SEEDS = int(os.environ.get("SCV_FUZZ_BOOT_MIXED", "20"))
SEQUENCE = 10
MIXED_WORK_DIV = 5
GUARD = 64                                                               # int64 words before and after the table of a DEVICE-mode call
PATTERN = -0x5A5A5A5A5A5A5A5B
CELL_FIELDS = ("max_count", "truth_count", "n_modes", "min_mode", "hit")


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cells_dev(cells):
    return _dev(np.ascontiguousarray(cells).view(np.uint8).reshape(cells.shape[0], cells.shape[1], 16))


def error_word(eng):
    import torch
    word = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    eng.export_error_word(word)
    return int(word.item())


def oracle_of(c):
    rc, want = coracle.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
    assert rc in (0, _lib.ERR_ARG)
    return rc, want


def queue_device(eng, c):
    """The case as a DEVICE-mode call into the middle of a prefilled buffer: enqueued only."""
    import torch
    big = torch.full((c.R * c.B * c.M + 2 * GUARD,), PATTERN, dtype=torch.int64, device="cuda")
    eng.bootstrap_device(cells_dev(c.cells), c.r_begin, c.r_end, c.seed64, c.M, out=big[GUARD:])
    return big


def assert_device_table(c, big, want):
    """The table was overwritten, whatever it held, and nothing around it was touched."""
    got = big.cpu().numpy()
    assert (got[:GUARD] == PATTERN).all() and (got[GUARD + want.size:] == PATTERN).all(), bf.describe(c)
    assert np.array_equal(got[GUARD:GUARD + want.size].reshape(want.shape), want), bf.describe(c)


def run_case(eng, c):
    rc, want = oracle_of(c)
    eng.set_option("boot_path", c.boot_path)
    try:
        if c.device:
            big = queue_device(eng, c)
            left = error_word(eng)                                       # in stream order behind the call: what it left in the word
            if rc == 0:
                eng.sync()
                assert left == 0, (bf.describe(c), left)
            else:
                assert left == 2, (bf.describe(c), left)
                with pytest.raises(_lib.ScvError) as e:
                    eng.sync()
                assert not isinstance(e.value, _lib.DomainError), bf.describe(c)
                eng.sync()                                               # the next one is clean
            assert_device_table(c, big, want)                            # (a hit that does not fit is left out of the table by the oracle too)
        elif rc == 0:
            got = eng.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
            assert got.shape == want.shape and np.array_equal(got, want), bf.describe(c)
        else:
            with pytest.raises(_lib.ScvError) as e:
                eng.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
            assert not isinstance(e.value, _lib.DomainError), bf.describe(c)
            eng.sync()                                                   # reported at the call: nothing is left for sync
    except _lib.ScvError as e:
        raise AssertionError(f"{bf.describe(c)}: {e}")
    finally:
        eng.set_option("boot_path", 0)
    assert error_word(eng) == 0, bf.describe(c)


# ---- 1. seeded calls ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(FIRST, FIRST + BOOT_SEEDS))
def test_random_bootstrap_call_is_bit_exact(hip_engine, seed):
    c = bf.draw(seed)
    if seed % 3 != 2:
        return run_case(hip_engine, c)
    from o1_inference_scaling_laws_amd.engine import Engine
    eng = Engine(timing=bool(seed & 1))                                  # the first call of a fresh context: every allocation on its path
    try:
        run_case(eng, c)
    finally:
        eng.close()


def test_resample_counts_around_the_cu_count(hip_engine):
    """R = CUs - 1, CUs, CUs + 1 and 2 CUs + 1 of THIS device: the grid of scv_bootstrap_lds_k is min(CUs, R), so these are a grid one short of
    the chip, exactly one resample per workgroup, one workgroup with a second turn, and a third turn for one alone; in both modes."""
    cases = bf.cu_cases(hip_engine.num_cus)
    assert {c.R for c in cases} == {hip_engine.num_cus + d for d in (-1, 0, 1)} | {2 * hip_engine.num_cus + 1}
    for i, c in enumerate(cases):
        c.device = bool(i & 1)
        run_case(hip_engine, c)


# ---- 2. both kernels on one draw ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(FIRST, FIRST + 40))
def test_both_kernels_give_one_table(hip_engine, seed):
    c = bf.draw(seed, clean=True)
    tables = []
    try:
        for path in (0, 3):
            hip_engine.set_option("boot_path", path)
            tables.append(hip_engine.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M))
    finally:
        hip_engine.set_option("boot_path", 0)
    assert np.array_equal(tables[0], tables[1]), bf.describe(c)
    assert np.array_equal(tables[0], oracle_of(c)[1]), bf.describe(c)


# ---- 3. slices concatenate ---------------------------------------------------------------------------------------------------------------------

def _slice_cases():
    some = bf.find(lambda c: c.R >= 2 and not c.overflow, 6)
    top = bf.find(lambda c: c.R >= 5 and c.P >= 64 and not c.overflow and c.r_end == bf.R_TOP, 2)
    return some + top


@pytest.mark.parametrize("path", [0, 3])
def test_slices_of_the_range_concatenate(hip_engine, path):
    """[r_begin, cut) and [cut, r_end) are the one table, cut; the cut is random, and two of the draws end at r_end = 2^31 - 1."""
    cases = _slice_cases()
    assert sum(c.r_end == bf.R_TOP for c in cases) >= 2
    hip_engine.set_option("boot_path", path)
    try:
        for c in cases:
            cut = c.r_begin + int(np.random.default_rng((77, c.seed)).integers(1, c.R))
            whole = hip_engine.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
            parts = [hip_engine.bootstrap(c.cells, a, b, c.seed64, c.M) for a, b in ((c.r_begin, cut), (cut, c.r_end))]
            assert np.array_equal(np.concatenate(parts, axis=0), whole), (bf.describe(c), cut)
            assert np.array_equal(whole, oracle_of(c)[1]), bf.describe(c)
    finally:
        hip_engine.set_option("boot_path", 0)


# ---- 4. vote and bootstrap in one call ---------------------------------------------------------------------------------------------------------

def fused_inputs(c):
    """Votes, truth, the oracle's aggregate and (M, resample table) of a draw_fused case."""
    a, _, tr = coracle.synth_fill(c.P, c.B, c.N, c.synth_seed, c.dist)
    want = coracle.aggregate(a, tr)
    M = int(want["cells"]["n_modes"][want["cells"]["hit"] == 1].max(initial=0)) + 1 + c.extra_classes
    rc, boot = coracle.bootstrap(want["cells"], c.r_begin, c.r_end, c.seed64, M)
    assert rc == 0
    return a, tr, want, M, boot


def call_fused(eng, c, a, tr, M):
    """The draw_fused case, enqueued under its two options (both back at their defaults afterwards)."""
    eng.set_option("boot_path", c.boot_path)
    eng.set_option("reg_n_max", c.reg_n_max)
    try:
        return eng.aggregate_bootstrap_device(_dev(a), _dev(tr), c.r_begin, c.r_end, c.seed64, M)
    finally:
        eng.set_option("boot_path", 0)
        eng.set_option("reg_n_max", bf.REG_N_MAX)


def assert_fused(c, out, want, boot):
    from o1_inference_scaling_laws_amd.engine import AggregateResult, cells_from_torch
    counters, cells, _, table = out
    gc = cells_from_torch(cells)
    for f in CELL_FIELDS:
        assert np.array_equal(gc[f], want["cells"][f]), (bf.describe(c), f)
    got = AggregateResult.from_counters(counters.cpu().numpy(), c.P, c.B)
    assert np.array_equal(got.tie_class_hits, want["tie_class_hits"]) and np.array_equal(got.truth_count_sum, want["truth_count_sum"]), bf.describe(c)
    assert np.array_equal(table.cpu().numpy(), boot), bf.describe(c)


def test_vote_and_bootstrap_in_one_call_on_random_shapes(hip_engine):
    """24 draws of scv_aggregate_bootstrap_i32 (4097 <= N <= 6000, P * B <= 600), half of them with two launches forced: cells, counters and
    the resample table against the oracle, ranges up to r_end = 2^31 - 1; the one-launch form and the two-launch form were both taken.  At
    these lengths the default dispatch runs the register-resident vote kernels, which never take the bootstrap into their launch: half of the
    unforced seeds select the streaming kernel (option "reg_n_max" = 4096, tests/_boot_fuzz.py draw_fused), the form with the grid barrier."""
    eng = hip_engine
    one0, two0 = eng.stat("boot_fused"), eng.stat("boot_separate")
    took, fused_at_the_top = {}, 0
    try:
        for seed in range(24):
            c = bf.draw_fused(seed)
            a, tr, want, M, boot = fused_inputs(c)
            f0, s0 = eng.stat("boot_fused"), eng.stat("boot_separate")
            out = call_fused(eng, c, a, tr, M)
            left = error_word(eng)
            eng.sync()
            assert left == 0, (bf.describe(c), left)
            assert_fused(c, out, want, boot)
            key = (c.boot_path, c.reg_n_max)
            took.setdefault(key, [0, 0])
            took[key][0] += eng.stat("boot_fused") - f0
            took[key][1] += eng.stat("boot_separate") - s0
            fused_at_the_top += c.r_end == bf.R_TOP and c.R >= 2 and eng.stat("boot_fused") > f0
    finally:
        eng.set_option("boot_path", 0)
        eng.set_option("reg_n_max", bf.REG_N_MAX)
    assert took[(2, bf.REG_N_MAX)] == [0, 12], took                      # two launches where the option asks for them
    assert took[(0, bf.REG_N_MAX)] == [0, 6], took                       # register-resident cells: the bootstrap is queued behind the vote
    assert took[(0, 4096)][0] >= 1 and sum(took[(0, 4096)]) == 6, took   # the streaming kernel: one launch wherever the table fits its LDS
    assert fused_at_the_top >= 1                                         # the loop behind the grid barrier ran up to r = 2^31 - 2
    assert eng.stat("boot_fused") > one0 and eng.stat("boot_separate") > two0


# ---- 5. who owns the error word ----------------------------------------------------------------------------------------------------------------

def _poisoned_votes():
    a, _, tr = synth.fill(6, 2, 40, 11, 1)
    a = a.copy()
    a[3, 1, 0] = 4000
    return _dev(a), _dev(tr)


def _clean_table():
    c = bf.find(lambda c: not c.overflow and c.M >= 3 and c.R >= 2 and c.cells["hit"].any() and c.work <= 100_000, 1)[0]
    return c, oracle_of(c)[1]


def test_a_host_bootstrap_leaves_an_earlier_device_error_to_sync(hip_engine):
    """A DEVICE-mode aggregate with a vote of 4000, not synced, then a HOST bootstrap of a clean table: the bootstrap returns the right table,
    the sync behind it raises DomainError, the next one is clean.  (include/scvote.h: a DEVICE-mode error is reported at scv_sync; a HOST call
    reports its own data.)"""
    eng = hip_engine
    c, want = _clean_table()
    ans, tr = _poisoned_votes()
    eng.sync()
    for path in (0, 3):
        eng.set_option("boot_path", path)
        try:
            eng.aggregate_device(ans, tr)
            got = eng.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
        finally:
            eng.set_option("boot_path", 0)
        assert np.array_equal(got, want)
        with pytest.raises(_lib.DomainError):
            eng.sync()
        eng.sync()
        assert error_word(eng) == 0


def test_a_host_bootstrap_reports_its_own_overflow_and_only_that(hip_engine):
    """The same pending bit, then a HOST bootstrap whose M is too small: ScvError -- not DomainError -- at the call, and the DEVICE call's
    DomainError is still delivered at sync."""
    eng = hip_engine
    c, _ = _clean_table()
    top = int(c.cells["n_modes"][c.cells["hit"] == 1].max())
    ans, tr = _poisoned_votes()
    eng.sync()
    eng.aggregate_device(ans, tr)
    with pytest.raises(_lib.ScvError) as e:
        eng.bootstrap(c.cells, 0, 64, c.seed64, top)
    assert not isinstance(e.value, _lib.DomainError)
    with pytest.raises(_lib.DomainError):
        eng.sync()
    eng.sync()
    assert error_word(eng) == 0
    # and with nothing pending the overflow leaves nothing behind
    with pytest.raises(_lib.ScvError):
        eng.bootstrap(c.cells, 0, 64, c.seed64, top)
    eng.sync()
    assert error_word(eng) == 0


def test_with_the_clamp_flag_neither_call_raises():
    from o1_inference_scaling_laws_amd.engine import Engine
    c, want = _clean_table()
    ans, tr = _poisoned_votes()
    with Engine(clamp_to_invalid_bin=True) as eng:
        eng.aggregate_device(ans, tr)
        assert np.array_equal(eng.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M), want)
        eng.sync()
        eng.sync()


# ---- 6. mixed sequences ------------------------------------------------------------------------------------------------------------------------

KINDS = ("boot_host", "boot_device", "aggregate_bootstrap", "aggregate", "lane")


def sequence_of(seed):
    """The 10 calls of sequence ``seed`` (no GPU): [(kind, case)], and the index of the poisoned call or -1."""
    from tests import test_gpu_fuzz_votes as fv
    rng = np.random.default_rng((9_400_000, seed))
    kinds = [KINDS[int(k)] for k in rng.integers(0, len(KINDS), size=SEQUENCE)]
    for k in range(len(KINDS)):                                          # every kind is in every sequence, wherever it falls
        if KINDS[k] not in kinds:
            kinds[int(rng.integers(0, SEQUENCE))] = KINDS[k]
    poisoned = 4 + seed % 3 if seed % 4 == 1 else -1
    if poisoned >= 0:
        kinds[poisoned] = "aggregate"
        if not any(k == "boot_host" for k in kinds[poisoned + 1:]):
            kinds[poisoned + 1] = "boot_host"                            # a HOST bootstrap behind the pending bit
    cases = []
    for i, kind in enumerate(kinds):
        s = 1000 * seed + i
        if kind in ("boot_host", "boot_device"):
            c = bf.draw(s, work_div=MIXED_WORK_DIV, clean=True)
            c.device = kind == "boot_device"
        elif kind == "aggregate_bootstrap":
            c = bf.draw_fused(s)
        elif kind == "aggregate":
            c = fv.draw_aggregate("aggregate", s)
            if i == poisoned:
                c.device = True
                c.pool = c.pool.copy()
                c.pool[int(rng.integers(0, c.P)), ..., 0] = int(rng.choice([-1, 1024, 4096]))
                fv.reach_first_vote(c)
        else:
            c = vf.draw(vf.LANE_ENTRIES[int(rng.integers(0, len(vf.LANE_ENTRIES)))], s, work_div=MIXED_WORK_DIV)
            c.grid = 0
        cases.append((kind, c))
    return cases, poisoned


@pytest.mark.parametrize("seed", range(FIRST, FIRST + MIXED_SEEDS))
def test_bootstrap_calls_interleaved_on_one_context(seed):
    """10 calls on one fresh context: HOST bootstrap, DEVICE bootstrap, vote + bootstrap, aggregate and one of the lane-body votes, modes mixed.
    HOST calls are checked as they return, DEVICE calls after ONE sync at the end.  One sequence in four carries an out-of-domain vote in a DEVICE
    aggregate in the middle, with a HOST bootstrap behind it: every other call is exact and only the sync raises."""
    from o1_inference_scaling_laws_amd.engine import Engine
    from tests import test_gpu_fuzz_votes as fv
    from tests._adapters import assert_results_equal
    cases, poisoned = sequence_of(seed)
    eng = Engine(timing=bool(seed & 1))
    queued = []
    try:
        for i, (kind, c) in enumerate(cases):
            where = (seed, i, kind)
            try:
                if kind in ("boot_host", "boot_device"):
                    rc, want = oracle_of(c)
                    assert rc == 0
                    eng.set_option("boot_path", c.boot_path)
                    if c.device:
                        queued.append((kind, c, want, queue_device(eng, c), None))
                    else:
                        got = eng.bootstrap(c.cells, c.r_begin, c.r_end, c.seed64, c.M)
                        assert np.array_equal(got, want), (where, bf.describe(c))
                    eng.set_option("boot_path", 0)
                elif kind == "aggregate_bootstrap":
                    a, tr, want, M, boot = fused_inputs(c)
                    queued.append((kind, c, want, call_fused(eng, c, a, tr, M), boot))
                elif kind == "aggregate":
                    want = fv.aggregate_want(c) if i != poisoned else None
                    if c.device:
                        queued.append((kind if i != poisoned else "poisoned", c, want, fv.aggregate_device(eng, c), None))
                    else:
                        assert_results_equal(fv.aggregate_host(eng, c), want, check_tokens=c.with_tokens)
                else:
                    want = vf.mirror_outputs(c)
                    if c.device:
                        bufs, prev = fv.previous_buffers(c, want, np.random.default_rng((57, seed, i)))
                        fv.device_call(eng, c, bufs)
                        queued.append((kind, c, want, bufs, prev))
                    else:
                        fv.assert_outputs(c, vf.outputs_of(c, fv.host_call(eng, c)), want)
            except _lib.ScvError as e:                                   # every call is valid, and a HOST call reports its own data only
                raise AssertionError(f"{where}: {e}")
        if poisoned >= 0:
            with pytest.raises(_lib.DomainError):
                eng.sync()
        eng.sync()                                                       # the one sync of the sequence (the second, clean one after an error)
        assert error_word(eng) == 0
        for kind, c, want, out, extra in queued:
            if kind == "boot_device":
                assert_device_table(c, out, want)
            elif kind == "aggregate_bootstrap":
                assert_fused(c, out, want, extra)
            elif kind == "aggregate":
                assert_results_equal(fv.aggregate_got(c, out), want, check_tokens=c.with_tokens)
            elif kind == "lane":
                fv.assert_outputs(c, fv.device_outputs(out), want, extra)
    finally:
        eng.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------

def _table(P, B, top, seed=3):
    rng = np.random.default_rng(seed)
    cells = np.zeros((P, B), dtype=coracle.CELL_DTYPE)
    cells["hit"] = rng.random((P, B)) < 0.6
    cells["n_modes"] = rng.integers(1, top + 1, size=(P, B))
    return cells


@pytest.mark.parametrize("B,M", [(1, 16385), (16, 1025), (5, 3277)])
def test_more_than_16384_counters_are_refused_at_the_call(hip_engine, B, M):
    import torch
    eng = hip_engine
    cells = _table(50, B, 2)
    with pytest.raises(_lib.ScvError):
        eng.bootstrap(cells, 0, 2, 1, M)
    out = torch.full((2 * B * M,), PATTERN, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.ScvError):
        eng.bootstrap_device(cells_dev(cells), 0, 2, 1, M, out=out)
    eng.sync()                                                           # refused at the call: nothing was queued, nothing is pending
    assert error_word(eng) == 0 and bool((out == PATTERN).all())


@pytest.mark.parametrize("B,M", bf.BM_PAIRS)
def test_exactly_16384_counters_are_accepted_and_exact(hip_engine, B, M):
    eng = hip_engine
    cells = _table(300, B, min(M - 1, 1024))
    c = bf.with_range(bf.draw(0), bf.R_TOP - 3, bf.R_TOP)
    c.cells, c.P, c.B, c.M, c.seed64 = cells, 300, B, M, 2 ** 64 - 1
    rc, want = oracle_of(c)
    assert rc == 0 and want.any()
    for path in (0, 3):
        eng.set_option("boot_path", path)
        try:
            assert np.array_equal(eng.bootstrap(cells, c.r_begin, c.r_end, c.seed64, M), want)
            big = queue_device(eng, c)
            eng.sync()
        finally:
            eng.set_option("boot_path", 0)
        assert_device_table(c, big, want)


@pytest.mark.parametrize("r_begin,r_end,M,P", [(-1, 3, 4, 20), (5, 4, 4, 20), (0, 3, 0, 20), (0, 3, 4, 0), (-(2 ** 31), 0, 4, 20)])
def test_bad_ranges_bounds_and_tables_are_refused(hip_engine, r_begin, r_end, M, P):
    import torch
    eng = hip_engine
    cells = _table(max(P, 1), 2, 2)[:P]
    out_host = np.zeros(64, dtype=np.int64)
    with pytest.raises(_lib.ScvError):
        _lib.check(eng._L.scv_bootstrap(eng._ctx, cells.ctypes.data, P, 2, r_begin, r_end, 1, M, _lib.MEM_HOST, out_host.ctypes.data))
    out = torch.full((64,), PATTERN, dtype=torch.int64, device="cuda")
    cd = cells_dev(_table(20, 2, 2))
    with pytest.raises(_lib.ScvError):
        _lib.check(eng._L.scv_bootstrap(eng._ctx, cd.data_ptr(), P, 2, r_begin, r_end, 1, M, _lib.MEM_DEVICE, out.data_ptr()))
    eng.sync()
    assert error_word(eng) == 0 and bool((out == PATTERN).all())
