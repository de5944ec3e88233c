"""The streaming kernel's dynamic item schedule: for items of at least 2^20 votes that outnumber the workgroups, a device counter hands
out every workgroup's items after its first instead of the round-robin stride (option path 0 .. 2; path 3 keeps the round-robin order).
The schedule changes which workgroup streams which cell, never what a cell's record or a budget's counters are: both schedules against
the C oracle, over unaligned rows, ragged budgets, every distribution with and without tokens, out-of-domain votes, split-N, the overwrite
and bootstrap forms, and launches back to back on one context (the counter must be zero again for the next launch).  Small grids
("grid") put more items than workgroups into shapes small enough to check.

Run on the GPU box:  python -m pytest tests/test_gpu_stream_schedule.py -m gpu -q
"""
import contextlib

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib
from o1_inference_scaling_laws_amd.engine import AggregateResult, Engine, cells_from_torch, counters_size
from oracle import coracle
from tests._adapters import OracleEngine, assert_results_equal

pytestmark = pytest.mark.gpu

FIELDS = ("max_count", "truth_count", "n_modes", "min_mode", "hit")


@contextlib.contextmanager
def engine(path, grid, clamp=False, **opts):
    """A fresh context on the streaming kernel: path 1 (whole cells, dynamic items), 2 (split-N) or 3 (whole cells, round-robin), `grid` workgroups."""
    with Engine(clamp_to_invalid_bin=clamp) as eng:
        eng.set_option("path", path)
        eng.set_option("grid", grid)
        for k, v in opts.items():
            eng.set_option(k, v)
        yield eng


def oracle(a, tr, t=None, nv=None, clamp=False):
    if clamp:
        want = coracle.aggregate(a, tr, tokens=t, n_valid=nv, clamp=True)
        assert want["rc"] == 0
        return want
    return OracleEngine().aggregate(a, tr, tokens=t, n_valid=nv)


@pytest.mark.parametrize("path", [1, 3])
@pytest.mark.parametrize("shape,grid", [((3, 3, 1 << 20), 4),          # 9 cells of 2^20 votes over 4 workgroups (not a multiple of the grid)
                                        ((5, 2, (1 << 20) + 1), 3),    # unaligned rows long enough for the counter
                                        ((3, 3, (1 << 20) + 3), 7),
                                        ((30, 3, 8193), 7),            # unaligned rows below 2^20 votes: round-robin on every path
                                        ((20, 4, 12345), 9)])
def test_dynamic_items_match_oracle(shape, grid, path):
    P, B, N = shape
    a, t, tr = coracle.synth_fill(P, B, N, 71, 1, want_tokens=True)
    with engine(path, grid) as eng:
        for rep in range(2):                        # back to back on one context
            assert_results_equal(eng.aggregate(a, tr, tokens=t), oracle(a, tr, t))
        assert_results_equal(eng.aggregate(a, tr), oracle(a, tr), check_tokens=False)


@pytest.mark.parametrize("tokens", [True, False])
@pytest.mark.parametrize("dist", [0, 1, 2, 3, 4, 5])
def test_dynamic_items_every_distribution(dist, tokens):
    P, B, N = 3, 2, (1 << 20) + 1
    a, t, tr = coracle.synth_fill(P, B, N, 500 + dist, dist, want_tokens=True)
    with engine(1, 4) as eng:
        got = eng.aggregate(a, tr, tokens=t if tokens else None)
    assert_results_equal(got, oracle(a, tr, t if tokens else None), check_tokens=tokens)


@pytest.mark.parametrize("path", [1, 3])
def test_dynamic_items_ragged_budgets(path):
    P, B, N = 2, 6, (1 << 20) + 3
    a, t, tr = coracle.synth_fill(P, B, N, 9, 1, want_tokens=True)
    nv = np.array([N, 1, 0, 1 << 19, 4099, N + 20000], dtype=np.int32)
    with engine(path, 5) as eng:
        assert_results_equal(eng.aggregate(a, tr, tokens=t, n_valid=nv), oracle(a, tr, t, nv))


def test_dynamic_items_domain_error_and_clamp():
    P, B, N = 3, 2, (1 << 20) + 3
    a, _, tr = coracle.synth_fill(P, B, N, 3, 1, want_tokens=True)
    a[1, 1, 400000] = 2000
    a[2, 0, 17] = -1
    with engine(1, 4) as eng:
        with pytest.raises(_lib.DomainError):
            eng.aggregate(a, tr)
        clean = np.minimum(np.abs(a), 1023)
        assert_results_equal(eng.aggregate(clean, tr), oracle(clean, tr), check_tokens=False)   # and the next launch is clean
    with engine(1, 4, clamp=True) as eng:
        got = eng.aggregate(a, tr)
    want = oracle(a, tr, clamp=True)
    for f in FIELDS:
        assert np.array_equal(got.cells[f], want["cells"][f]), f


def test_dynamic_items_split_n():
    """Split-N items (segments of 2^20 votes merged inside the launch) handed out by the counter: 3 cells x 4 segments over 5 workgroups."""
    P, B, N = 3, 1, 1 << 22
    a, t, tr = coracle.synth_fill(P, B, N, 13, 1, want_tokens=True)
    with engine(2, 5, segs=4) as eng:
        for rep in range(2):
            assert_results_equal(eng.aggregate(a, tr, tokens=t), oracle(a, tr, t))


@pytest.mark.parametrize("path", [1, 3])
def test_dynamic_items_overwrite_and_bootstrap(path):
    import torch
    P, B, N = 10, 2, 1 << 20
    dev = torch.device("cuda:0")
    a, t, tr = coracle.synth_fill(P, B, N, 77, 1, want_tokens=True)
    want = coracle.aggregate(a, tr, tokens=t)
    M = int(want["cells"]["n_modes"][want["cells"]["hit"] == 1].max(initial=0)) + 1
    rc, want_boot = coracle.bootstrap(want["cells"], 2, 131, 99, M)
    assert rc == 0
    ad, td, trd = (torch.from_numpy(x).to(dev) for x in (a, t, tr))
    with engine(path, 6) as eng:
        for rep in range(2):                        # overwrite: the last workgroup turns the cell table into the counters
            counters = torch.full((counters_size(B),), -5 - rep, dtype=torch.int64, device=dev)
            c, cells, ctok = eng.aggregate_device(ad, trd, tokens=td, counters=counters, overwrite=True)
            eng.sync()
            got = AggregateResult.from_counters(c.cpu().numpy(), P, B)
            assert np.array_equal(got.tie_class_hits, want["tie_class_hits"]) and np.array_equal(got.token_sum, want["token_sum"])
            assert np.array_equal(got.truth_count_sum, want["truth_count_sum"])
            gc = cells_from_torch(cells)
            for f in FIELDS:
                assert np.array_equal(gc[f], want["cells"][f]), f
            assert np.array_equal(ctok.cpu().numpy(), want["cell_tokens"])
        for rep in range(2):                        # vote + bootstrap in one launch (grid barrier after the last item)
            counters, cells, _, boot = eng.aggregate_bootstrap_device(ad, trd, 2, 131, 99, M)
            eng.sync()
            gc = cells_from_torch(cells)
            for f in FIELDS:
                assert np.array_equal(gc[f], want["cells"][f]), f
            assert np.array_equal(AggregateResult.from_counters(counters.cpu().numpy(), P, B).tie_class_hits, want["tie_class_hits"])
            assert np.array_equal(boot.cpu().numpy(), want_boot)


def test_dynamic_items_device_launches_back_to_back():
    """Several DEVICE-mode launches queued on one context without a sync between them, on different inputs: each must start
    from a zero counter (the previous launch's last ticket cleared it)."""
    import torch
    P, B, N = 4, 2, 1 << 20
    dev = torch.device("cuda:0")
    with engine(1, 3) as eng:
        ins, outs = [], []
        for s in range(4):
            a, _, tr = coracle.synth_fill(P, B, N, 1000 + s, s % 6, want_tokens=True)
            ad, trd = torch.from_numpy(a).to(dev), torch.from_numpy(tr).to(dev)
            outs.append(eng.aggregate_device(ad, trd))
            ins.append((a, tr, ad, trd))
        eng.sync()
        for (a, tr, _, _), (c, cells, _) in zip(ins, outs):
            want = oracle(a, tr)
            gc = cells_from_torch(cells)
            for f in FIELDS:
                assert np.array_equal(gc[f], want.cells[f]), f
            assert np.array_equal(AggregateResult.from_counters(c.cpu().numpy(), P, B).tie_class_hits, want.tie_class_hits)


def test_path_option_range():
    with Engine() as eng:
        for v in range(6):
            eng.set_option("path", v)
        with pytest.raises(_lib.ScvError):
            eng.set_option("path", 6)
