"""DEVICE-mode scv_aggregate_i32 / scv_aggregate_prefix_i32 inside guard bands (tests/_agg_guard.py): every tensor of a call is a view into ONE
dirty byte arena, the outputs at the documented alignment and nothing more, and after the call the whole arena is compared byte for byte with what
oracle.coracle says it must hold -- a record past a table, a vector store over a ragged tail, a table nobody asked for or a counted guard vote
all show.  Also here: what a packed context and a misaligned output are refused (include/scvote.h), with nothing queued."""
import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib
from tests import _agg_guard as G

pytestmark = pytest.mark.gpu

_PACKED = {}


def _packed_engine():
    if "eng" not in _PACKED:
        from o1_inference_scaling_laws_amd.engine import Engine
        _PACKED["eng"] = Engine(packed_cells=True)
    return _PACKED["eng"]


def _views(c, regions, dev_arena):
    import torch
    def view(name, dtype, shape):                       # noqa: E306
        o, n = regions[name]
        return dev_arena[o:o + n].view(dtype).view(shape)
    ncells_shape = (c.P, c.B)
    return dict(votes=view("votes", torch.int32, c.votes.shape), truth=view("truth", torch.int32, (c.P,)),
                tokens=view("tokens", torch.int32, c.votes.shape) if c.tokens_on else None,
                n_valid=view("n_valid", torch.int32, (c.B,)) if c.n_valid is not None else None,
                counters=view("counters", torch.int64, (G.counters_size(c.B),)),
                cells=view("cells", torch.uint8, (*ncells_shape, 4 if c.packed else 16)) if c.want_cells else False,
                cell_tokens=view("cell_tokens", torch.int64, ncells_shape) if c.ctok_given else None)


def _launch(eng, c, v):
    """Queues the call; no synchronisation."""
    if c.prefix:
        eng.aggregate_prefix_device(v["votes"], v["truth"], v["n_valid"], tokens=v["tokens"], counters=v["counters"], cells=v["cells"],
                                    cell_tokens=v["cell_tokens"], overwrite=c.overwrite, budgets_host=c.budgets if c.budgets_host else None)
    else:
        eng.aggregate_device(v["votes"], v["truth"], tokens=v["tokens"], n_valid=v["n_valid"], counters=v["counters"], cells=v["cells"],
                             cell_tokens=v["cell_tokens"], overwrite=c.overwrite)


def _prepare(c):
    import torch
    regions, size = G.layout(c)
    arena = G.host_arena(c, regions, size)
    want = G.expected_arena(c, regions, arena, G.oracle_outputs(c))
    dev = torch.from_numpy(arena).to(torch.device("cuda:0"))
    assert dev.data_ptr() % 256 == 0
    return regions, want, dev


def _restore(eng):
    for k, v in G.OPTION_DEFAULTS:
        eng.set_option(k, v)


@pytest.mark.parametrize("seed", range(G.DEFAULT_SEEDS))
def test_a_call_inside_guard_bands_leaves_the_oracles_bytes_and_nothing_else(hip_engine, seed):
    c = G.draw(seed)
    eng = _packed_engine() if c.packed else hip_engine
    regions, want, dev = _prepare(c)
    try:
        for k, v in c.opts.items():
            eng.set_option(k, v)
        _launch(eng, c, _views(c, regions, dev))
        err = 0
        try:
            eng.sync()
        except _lib.ScvError as e:
            err = str(e)
    finally:
        _restore(eng)
    assert not err, f"seed {seed} ({c.stratum}): {err}"
    G.check(c, regions, want, dev.cpu().numpy())


def test_eight_mixed_calls_back_to_back_without_a_sync_between_them(hip_engine):
    """Dense and prefix, every kernel kind, both contexts' record forms on one context each: queued one behind the other, checked at the end."""
    n = len(G.STRATA)
    seeds = [s for s in (0, 9, 15, 25, 34, 38, 43, 45, n + 3, n + 12, n + 30, n + 41) if not G.draw(s).packed][:8]
    assert len(seeds) == 8
    queued = []
    try:
        for s in seeds:
            c = G.draw(s)
            regions, want, dev = _prepare(c)
            for k, v in G.OPTION_DEFAULTS:
                hip_engine.set_option(k, c.opts.get(k, v))
            _launch(hip_engine, c, _views(c, regions, dev))
            queued.append((c, regions, want, dev))
        hip_engine.sync()
    finally:
        _restore(hip_engine)
    assert len({c.stratum for c, *_ in queued}) == 8
    for c, regions, want, dev in queued:
        G.check(c, regions, want, dev.cpu().numpy())


# ---- refusals (written for the library that has them: on a library without them the first three are an out-of-bounds device write) -----------------

def _packed_case(N, tokens=False):
    import torch
    from oracle import coracle
    P, B = 37, 3
    a, t, tr = coracle.synth_fill(P, B, N, 4242 + N, 1, want_tokens=True)
    dev = torch.device("cuda:0")
    arena = torch.full((4096 + 4 * P * B,), G.PATTERN, dtype=torch.uint8, device=dev)
    table = arena[2048:2048 + 4 * P * B].view(P, B, 4)
    return a, tr, torch.from_numpy(a).to(dev), torch.from_numpy(tr).to(dev), arena, table


@pytest.mark.parametrize("N,opts", [(100, {"reg_n_max": 99}), (40, {"sort_n_max": 0, "reg_n_max": 39}), (100, {"reg_shape": 1041})],
                         ids=["stream_100", "stream_40_sort_off", "dense_100"])
def test_a_packed_context_refuses_the_kernels_that_write_16_byte_records(N, opts):
    import torch
    from oracle import coracle
    from o1_inference_scaling_laws_amd.engine import cells_from_torch
    eng = _packed_engine()
    a, tr, da, dtr, arena, table = _packed_case(N)
    want = coracle.aggregate(a, tr)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        with pytest.raises(_lib.ScvError):
            eng.aggregate_device(da, dtr, cells=table)
        eng.sync()
        assert bool((arena == G.PATTERN).all())                                  # the table's pattern and its guards: nothing was queued
        c, none, _ = eng.aggregate_device(da, dtr, cells=False)                   # counters only: every kernel serves a packed context
        eng.sync()
        assert none is None and np.array_equal(c.cpu().numpy()[: 3 * 1025], want["tie_class_hits"].reshape(-1))
        assert np.array_equal(c.cpu().numpy()[3 * 1025 + 3:], want["truth_count_sum"])
        assert bool((arena == G.PATTERN).all())
    finally:
        _restore(eng)
    _, cells, _ = eng.aggregate_device(da, dtr, cells=table)                      # the same context serves the next default call, into the same table
    eng.sync()
    got = cells_from_torch(cells)
    for f in ("max_count", "truth_count", "n_modes", "min_mode", "hit"):
        assert np.array_equal(got[f], want["cells"][f]), f
    assert bool((arena[:2048] == G.PATTERN).all()) and bool((arena[2048 + table.numel():] == G.PATTERN).all())
    assert torch.equal(table, cells)


@pytest.mark.parametrize("which,offset", [("cells", 4), ("cells", 8), ("cell_tokens", 8), ("counters", 4)])
def test_an_output_below_its_alignment_is_refused_with_nothing_queued(hip_engine, which, offset):
    """cells_out / cell_tokens_out need 16 bytes, the counters 8 (include/scvote.h): the widest store each receives."""
    import ctypes as C
    import torch
    from oracle import coracle
    P, B, N = 20, 2, 8
    a, t, tr = coracle.synth_fill(P, B, N, 77, 1, want_tokens=True)
    dev = torch.device("cuda:0")
    da, dt, dtr = (torch.from_numpy(x).to(dev) for x in (a, t, tr))
    arena = torch.full((1 << 16,), G.PATTERN, dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    ptr = {"cells": base + 1024, "cell_tokens": base + 8192, "counters": base + 16384}
    ptr[which] += offset
    cnt = ptr["counters"]
    hip_engine.use_torch_stream()
    L = hip_engine._L
    rc = L.scv_aggregate_i32(hip_engine._ctx, C.c_void_p(da.data_ptr()), C.c_void_p(dt.data_ptr()), None, C.c_void_p(dtr.data_ptr()), P, B, N, _lib.MEM_DEVICE,
                             C.c_void_p(ptr["cells"]), C.c_void_p(ptr["cell_tokens"]), C.c_void_p(cnt), C.c_void_p(cnt + 8 * B * 1025),
                             C.c_void_p(cnt + 8 * (B * 1025 + B)))
    assert rc == -2001                                                            # SCV_ERR_ARG
    rc = L.scv_aggregate_prefix_i32(hip_engine._ctx, C.c_void_p(da.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(dtr.data_ptr()), C.c_void_p(dtr.data_ptr()),
                                    P, 1, B * N, _lib.MEM_DEVICE, C.c_void_p(ptr["cells"]), C.c_void_p(ptr["cell_tokens"]), C.c_void_p(cnt),
                                    C.c_void_p(cnt + 8 * 1025), C.c_void_p(cnt + 8 * 1026))
    assert rc == -2001
    hip_engine.sync()
    assert bool((arena == G.PATTERN).all())
