"""CPU tests of the open answer domain (SCV_FLAG_OPEN_DOMAIN, include/scvote.h) on the numpy mirrors: with ``open_domain=True`` a mirror on
(pool, truth) of arbitrary int32 equals itself with ``open_domain=False`` on the order-preserving relabelling of the rows, in every output; the
value classes really hold what they promise; decode_min_mode inverts the code rule.  The device encoder ranks by counting (no sorting network,
nothing host-side to compile): its algorithm -- votes below each key, then dense ranks of those counts -- is checked here in numpy."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib
from o1_inference_scaling_laws_amd.engine import decode_min_mode
from o1_inference_scaling_laws_amd.resample import dense_codes, truth_codes
from tests import _open_domain as od


def test_the_flag_is_a_free_bit():
    assert _lib.FLAG_OPEN_DOMAIN == 0x8
    assert len({_lib.FLAG_TIMING, _lib.FLAG_CLAMP, _lib.FLAG_PACKED_CELLS, _lib.FLAG_OPEN_DOMAIN}) == 4


def test_value_classes_hold_what_they_promise():
    rng = np.random.default_rng(1)
    pool, truth = od.make_pool(rng, 60, 256)
    rows = {c: pool[i::len(od.CLASSES)] for i, c in enumerate(od.CLASSES)}
    assert all(len(np.unique(r)) == 1 for r in rows["equal"])
    assert all(len(np.unique(r)) == 256 for r in rows["distinct"])
    assert all(set(od.SPECIAL.tolist()) <= set(r.tolist()) for r in rows["special"])
    for r in rows["bitpairs"]:
        s = set(r.tolist())
        assert any((v ^ 1) in s for v in s) and any((v - 2 ** 31 in s) or (v + 2 ** 31 in s) for v in s)
    present = np.array([(pool[p] == truth[p]).any() for p in range(60)])
    assert present.any() and (~present).any() and (truth[present] == od.I32_MIN).any() and (truth[present] < 0).any()
    enc, tc = od.relabel(pool, truth)
    assert enc.max() == 255 and enc.min() == 0 and (tc[~present] == 1023).all() and (tc[present] < 256).all()


@pytest.mark.parametrize("N", [1, 4, 5, 64, 65, 129, 256])
def test_shared_row_encoder(N):
    rng = np.random.default_rng(N)
    pool, truth = od.make_pool(rng, 24, N)
    enc, tc = od.relabel(pool, truth)
    codes, uniq, bad = dense_codes(pool, open_domain=True)
    assert not bad and np.array_equal(codes, enc)
    assert all(np.array_equal(u, np.unique(pool[p])) for p, u in enumerate(uniq))
    t = truth_codes(uniq, truth, open_domain=True)
    assert np.array_equal(np.where(t < 0, 1023, t), tc)
    # without the parameter: the clamp and the flag, as before
    codes0, _, bad0 = dense_codes(pool)
    clamped = np.where((pool < 0) | (pool >= 1024), 1023, pool)
    assert bad0 == bool((clamped != pool).any()) and np.array_equal(codes0, od.relabel(clamped, truth)[0])


@pytest.mark.parametrize("N", od.NS)
def test_rank_by_counting_is_the_dense_rank(N):
    """What resample_encode_row_open computes: lt[e] = votes below key e (signed); the dense rank of lt is the dense rank of the keys."""
    rng = np.random.default_rng(100 + N)
    pool, _ = od.make_pool(rng, 18, N)
    for row in pool:
        lt = (row[None, :].astype(np.int64) < row[:, None].astype(np.int64)).sum(axis=1)
        assert lt.max() < N <= 256
        assert np.array_equal(np.unique(lt, return_inverse=True)[1].reshape(-1), np.unique(row, return_inverse=True)[1].reshape(-1))


@pytest.mark.parametrize("entry", od.ENTRIES)
def test_mirror_relabelling_invariance(entry):
    for c in od.grid_cases(entry):
        on = od.run_mirror(c, True)
        enc, tc = od.relabel(c["pool"], c["truth"])
        off = od.run_mirror(od.with_pool(c, enc, tc), False)
        assert on["err"] == 0 and off["err"] == 0
        od.assert_equal(on, off, (entry, c["N"], c["P"], c["R"]))


@pytest.mark.parametrize("entry", od.HAS_POOL_ORDER)
def test_min_mode_is_a_code_and_decodes_to_the_value(entry):
    rng = np.random.default_rng(5)
    c = od.make_case(rng, entry, 12, 65, None, B=4)
    c["pool"] = (c["pool"].astype(np.int64) % 1024).astype(np.int32)            # in-domain: the flag-off mirror reports values
    c["truth"] = (c["truth"].astype(np.int64) % 1024).astype(np.int32)
    on, off = od.run_mirror(c, True), od.run_mirror(c, False)
    od.assert_equal(on, off, entry, skip=("cells.min_mode",))
    vals = decode_min_mode(c["pool"], on["cells"])
    assert np.array_equal(vals, off["cells"]["min_mode"].astype(np.int64))
    empty = on["cells"]["max_count"] == 0
    assert empty.any() and (on["cells"]["min_mode"][empty] == -1).all() and (on["cells"]["min_mode"][~empty] >= 0).all()


def test_fuzz_draws_cover_the_sweep():
    seen = {(c["entry"], mode) for _, mode, c in od.fuzz_cases()}
    assert seen == {(e, m) for e in od.ENTRIES for m in ("host", "device")}
