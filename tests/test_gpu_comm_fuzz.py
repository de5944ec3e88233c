"""The one-process communicator (csrc/scvote_comm.hip) against the numpy model of tests/_comm_fuzz.py, whole backing arrays, bit for bit:
60 seeded sequences through the raw C ABI (collectives back to back on one buffer, torch writes between them on the ranks' streams, no host
sync before the one at the end) and the same 60 through ``MultiDeviceEngine`` (inputs produced by torch ops right before the collective
behind a long chain of work, no synchronize anywhere, every third seed on a fresh engine; after every collective each engine is bound to
torch's current stream); the growth of the staging buffer, with a call right behind it; a captured all-reduce replayed on new values and
the refusal to grow under capture; sixteen ranks; one rank (peer: nothing happens; RCCL: identity); a device error on one rank that travels
through the all-reduce; and C5 on shards without problems and without resamples.  Everything on device 0, in one process.

SCV_FUZZ_COMM_SEEDS and SCV_FUZZ_FIRST move the seed range."""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from o1_inference_scaling_laws_amd import _lib
from o1_inference_scaling_laws_amd.engine import AggregateResult, cells_from_torch, counters_size
from oracle import coracle
from tests import _comm_fuzz as cf

pytestmark = pytest.mark.gpu

FIRST = int(os.environ.get("SCV_FUZZ_FIRST", "0"))
SEEDS = range(FIRST, FIRST + int(os.environ.get("SCV_FUZZ_COMM_SEEDS", str(cf.DEFAULT_SEEDS))))
CHAIN_WORDS, CHAIN_OPS = 4_000_000, 200                                  # the work in front of a producer: an unordered stream overtakes it
CELL_FIELDS = ("max_count", "truth_count", "n_modes", "min_mode", "hit")


def create(G, flags=_lib.COMM_PEER):
    L = _lib.load()
    comm = C.c_void_p()
    _lib.check(L.scv_comm_create(C.byref(comm), (C.c_int * G)(*([0] * G)), G, 0, flags))
    return comm


def stat(comm, key):
    v = C.c_int64()
    _lib.check(_lib.load().scv_comm_get_stat(comm, key.encode(), C.byref(v)))
    return int(v.value)


def hand_built(G, W, ops, seed, off=3, full_range=True):
    """A sequence with fixed ops in the form of a draw (random values and guards)."""
    rng = np.random.default_rng((cf.STREAM + 1, seed))
    hi = 2 ** 63 if full_range else 1000
    return SimpleNamespace(seed=seed, G=G, off=off, W=W, ops=list(ops), value_kind="full" if full_range else "small", work=0,
                           init=[rng.integers(-hi, hi, size=off + W + cf.GUARD, dtype=np.int64) for _ in range(G)])


def upload(q):
    import torch
    return [torch.from_numpy(np.array(x)).to("cuda:0") for x in q.init]


def collective(L, comm, q, op, backs):
    """One collective of a sequence through the raw C ABI on the ranks' working buffers: enqueued only."""
    ptrs = (C.c_void_p * q.G)(*[b.data_ptr() + 8 * q.off for b in backs])
    if op[0] == "allreduce":
        _lib.check(L.scv_allreduce_counters(comm, ptrs, op[1]))
    elif op[0] == "allgather_i64":
        _lib.check(L.scv_allgather_i64(comm, ptrs, (C.c_int64 * q.G)(*op[1])))
    else:
        _lib.check(L.scv_allgather_cells(comm, ptrs, (C.c_int64 * q.G)(*op[1]), op[2]))


def assert_equal_to_model(q, backs, want=None):
    want = cf.model(q) if want is None else want
    for r, (b, w) in enumerate(zip(backs, want)):
        got = b.cpu().numpy()
        if not np.array_equal(got, w):
            bad = np.flatnonzero(got != w)
            raise AssertionError(f"rank {r}: {bad.size} words differ, first at word {bad[0] - q.off} of the working buffer (last {bad[-1] - q.off}): "
                                 f"got {got[bad[0]]} want {w[bad[0]]}; {cf.describe(q)}")


@pytest.fixture(scope="module")
def comms():
    """One communicator per rank count for the C-ABI sequences, destroyed behind the last test of the file."""
    cache = {}
    yield lambda G: cache.get(G) or cache.setdefault(G, create(G))
    for comm in cache.values():
        _lib.load().scv_comm_destroy(comm)


@pytest.fixture(scope="module")
def engines():
    from o1_inference_scaling_laws_amd.engine import MultiDeviceEngine
    cache = {}
    yield lambda G: cache.get(G) or cache.setdefault(G, MultiDeviceEngine(devices=[0] * G))
    for me in cache.values():
        me.close()


@pytest.fixture(scope="module")
def streams():
    import torch
    return [torch.cuda.Stream(device=0) for _ in range(max(cf.G_CHOICES))]


# ---- 1. sequences through the C ABI ------------------------------------------------------------------------------------------------

def run_c_abi(comm, q, rank_streams):
    """``rank_streams[r]``: the torch stream rank r's context is bound to (None: the device's default stream).  Writes go to the rank's
    stream; nothing synchronises between the first op and scv_comm_sync."""
    import torch
    L = _lib.load()
    for r, s in enumerate(rank_streams):
        _lib.check(L.scv_set_stream(L.scv_comm_ctx(comm, r), C.c_void_p(s.cuda_stream) if s is not None else None))
    backs = upload(q)
    torch.cuda.synchronize()                                             # the inputs exist; from here on the streams' own order has to do
    for op in q.ops:
        if op[0] == "write":
            s = rank_streams[op[1]]
            with torch.cuda.stream(s) if s is not None else contextlib.nullcontext():
                backs[op[1]][q.off:q.off + q.W].mul_(op[2]).add_(op[3])
        elif op[0] != "rebind":
            collective(L, comm, q, op, backs)
    _lib.check(L.scv_comm_sync(comm))
    return backs


def streams_of(seed, G, streams):
    """A stream of its own per rank / one stream for all / the default stream, in turn over the seeds."""
    return (streams[:G], [streams[0]] * G, [None] * G)[seed % 3]


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_through_the_c_abi(seed, comms, streams):
    q = cf.draw(seed)
    assert_equal_to_model(q, run_c_abi(comms(q.G), q, streams_of(seed, q.G, streams)))


# ---- 2. sequences through MultiDeviceEngine ----------------------------------------------------------------------------------------

def run_engine(me, q, side, chain):
    """The sequence through all_reduce_counters / all_gather_i64 / all_gather_cells with NO synchronize: every input of a collective is
    the output of a torch op queued right before it, behind CHAIN_OPS in-place ops over CHAIN_WORDS words on the same stream.
    Returns (backing tensors, [every engine bound to torch's current stream?] per collective)."""
    import torch
    src = upload(q)
    backs = [torch.empty_like(s) for s in src]

    def busy():
        for _ in range(CHAIN_OPS):
            chain.add_(1)

    busy()
    for b, s in zip(backs, src):
        b.copy_(s)                                                       # the producer of the first collective's input
    bufs = [b[q.off:q.off + q.W] for b in backs]
    main = torch.cuda.current_stream(0)
    on_side, bound = False, []
    for op in q.ops:
        if op[0] == "rebind":                                            # to the side stream, or back: the new stream continues where the old one is
            new, old = (main, side) if on_side else (side, main)
            new.wait_stream(old)
            on_side = not on_side
            continue
        with torch.cuda.stream(side) if on_side else contextlib.nullcontext():
            if op[0] == "write":
                busy()
                bufs[op[1]].mul_(op[2]).add_(op[3])
                continue
            if op[0] == "allreduce":
                me.all_reduce_counters([b[:op[1]] for b in bufs])
            elif op[0] == "allgather_i64":
                me.all_gather_i64(bufs, op[1])
            else:
                rows, B = sum(op[1]), op[2]
                me.all_gather_cells([b[:rows * B * 2].view(torch.uint8).view(rows, B, 16) for b in bufs], op[1])
            cur = int(torch.cuda.current_stream(0).cuda_stream)
            bound.append(all(e._bound_stream == cur for e in me.engines))
    if on_side:
        main.wait_stream(side)
    me.sync()
    return backs, bound


@pytest.fixture(scope="module")
def chain():
    import torch
    return torch.zeros(CHAIN_WORDS, dtype=torch.int64, device="cuda:0")


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_through_multi_device_engine(seed, engines, streams, chain):
    from o1_inference_scaling_laws_amd.engine import MultiDeviceEngine
    q = cf.draw(seed)
    fresh = seed % 3 == 0                                                # the first call of a new engine is the collective
    me = MultiDeviceEngine(devices=[0] * q.G) if fresh else engines(q.G)
    try:
        backs, bound = run_engine(me, q, streams[0], chain)
        assert all(bound), (bound, cf.describe(q))                       # the deterministic guard: no collective on a stream torch is not on
        assert_equal_to_model(q, backs)
    finally:
        if fresh:
            me.close()


# ---- 3. staging growth -------------------------------------------------------------------------------------------------------------

def run_steps(comm, q, steps):
    """``steps``: lists of ops; one scv_comm_sync and one whole comparison behind each list, nothing between the ops of a list."""
    import torch
    L = _lib.load()
    backs = upload(q)
    torch.cuda.synchronize()
    done = []
    for ops in steps:
        for op in ops:
            collective(L, comm, q, op, backs)
        _lib.check(L.scv_comm_sync(comm))
        done += ops
        assert_equal_to_model(SimpleNamespace(**{**vars(q), "ops": done}), backs)
        yield


def test_staging_buffer_grows_once_and_the_next_call_runs_on_the_grown_buffers():
    L = _lib.load()
    S = cf.STAGING_WORDS
    q = hand_built(3, 300_000 + 5, [], seed=1)
    comm = create(3)
    try:
        assert stat(comm, "staging_bytes") == 1 << 20
        steps = run_steps(comm, q, [[("allreduce", S)], [("allreduce", S + 1), ("allreduce", 8217)], [("allreduce", 300_000)]])
        next(steps)
        assert stat(comm, "staging_bytes") == 1 << 20                    # exactly the buffer of the create: no growth
        next(steps)
        assert stat(comm, "staging_bytes") == 8 * (S + 1)
        next(steps)
        assert stat(comm, "staging_bytes") == 8 * 300_000
    finally:
        L.scv_comm_destroy(comm)


def test_first_all_reduce_of_a_communicator_is_above_the_staging_buffer():
    L = _lib.load()
    q = hand_built(2, 200_003, [], seed=2, off=4)
    comm = create(2)
    try:
        next(run_steps(comm, q, [[("allreduce", 200_001), ("allgather_i64", (7, 190_000))]]))
        assert stat(comm, "staging_bytes") == 8 * 200_001
    finally:
        L.scv_comm_destroy(comm)


# ---- 4. capture --------------------------------------------------------------------------------------------------------------------

def test_captured_all_reduce_replays_on_new_values_and_growth_is_refused_under_capture():
    import torch
    from o1_inference_scaling_laws_amd.engine import MultiDeviceEngine
    n, big = 8217, cf.STAGING_WORDS + 1
    rng = np.random.default_rng(77)
    with MultiDeviceEngine(devices=[0, 0]) as me:
        bufs = [torch.zeros(n + 6, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        large = [torch.ones(big, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        views = [b[3:3 + n] for b in bufs]
        side = torch.cuda.Stream(device=0)
        side.wait_stream(torch.cuda.current_stream(0))
        with torch.cuda.stream(side):                                    # warm-up: both engines are bound to the capture stream from here on
            me.all_reduce_counters(views)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                           # one stream for both ranks: a graph without parallel branches
            with pytest.raises(_lib.ScvError) as e:
                me.all_reduce_counters(large)
            assert e.value.code == _lib.ERR_ARG and str(big) in str(e.value) and "captured" in str(e.value)
            me.all_reduce_counters(views)
        assert me.stat("staging_bytes") == 1 << 20
        for _ in range(3):
            vals = [rng.integers(-2 ** 63, 2 ** 63, size=n + 6, dtype=np.int64) for _ in range(2)]
            for b, v in zip(bufs, vals):
                b.copy_(torch.from_numpy(v))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            total = vals[0][3:3 + n].view(np.uint64) + vals[1][3:3 + n].view(np.uint64)
            for b, v in zip(bufs, vals):
                want = v.copy()
                want[3:3 + n] = total.view(np.int64)
                assert np.array_equal(b.cpu().numpy(), want)
        me.sync()
        assert all(int(x.sum()) == big for x in large)                   # the refused call touched nothing
        me.all_reduce_counters(large)                                    # outside the capture the same size grows the buffer
        me.sync()
        assert me.stat("staging_bytes") == 8 * big and all(int(x.sum()) == 2 * big for x in large)


# ---- 5. sixteen ranks --------------------------------------------------------------------------------------------------------------

def test_sixteen_ranks():
    L = _lib.load()
    G = 16                                                               # kMaxRanks; 17 are refused (test_c_abi_communicator_argument_errors)
    counts = (5, 0, 1000, 1, 0, 0, 77, 3000, 1, 1, 0, 256, 257, 0, 9, 0)
    q = hand_built(G, 16385 + 4, [], seed=3, off=4)
    comm = create(G)
    try:
        assert L.scv_comm_size(comm) == G
        assert stat(comm, "selftest_words") == 2 * (8217 * G + G * 1031)     # comm_selftest: two rounds of 8217 words from each of n ranks + n blocks of 1031
        assert stat(comm, "peer_loads") in (0, 1) and stat(comm, "staging_bytes") == 1 << 20
        next(run_steps(comm, q, [[("allreduce", 16385), ("allgather_i64", counts)]]))
    finally:
        L.scv_comm_destroy(comm)


# ---- 6. one rank -------------------------------------------------------------------------------------------------------------------

ONE_RANK_OPS = [("allreduce", 8217), ("allgather_i64", (100,)), ("allgather_cells", (7,), 3), ("allreduce", 16385)]


def test_one_peer_rank_leaves_everything_untouched():
    L = _lib.load()
    q = hand_built(1, 16385 + 2, [], seed=4)
    comm = create(1)
    try:
        assert stat(comm, "peer_loads") == -1 and stat(comm, "selftest_words") == 0
        next(run_steps(comm, q, [ONE_RANK_OPS]))                         # the model of one rank: the identity, guards included
    finally:
        L.scv_comm_destroy(comm)


def test_one_rccl_rank_is_the_identity(streams):
    L = _lib.load()
    ops = ONE_RANK_OPS[:2] + [("write", 0, -3, 12345)] + ONE_RANK_OPS[2:]
    q = hand_built(1, 16385 + 2, ops, seed=5, off=4)
    comm = create(1, _lib.COMM_RCCL)
    try:
        assert stat(comm, "peer_loads") == -1 and stat(comm, "selftest_words") > 0
        assert_equal_to_model(q, run_c_abi(comm, q, [streams[1]]))
    finally:
        L.scv_comm_destroy(comm)


# ---- 7. errors travel --------------------------------------------------------------------------------------------------------------

def test_a_device_error_on_one_rank_travels_through_the_all_reduce():
    import torch
    L = _lib.load()
    G, n, P, B, N = 3, 1000, 20, 2, 50
    q = hand_built(G, n + 1, [("allreduce", n), ("allreduce", n + 1)], seed=6)
    for x in q.init:
        x[q.off + n] = 0                                                 # the error word of the rank
    a, _, tr = coracle.synth_fill(P, B, N, 9, 1)
    a[7, 1, 13] = 1 << 20                                                # one vote outside the bins
    comm = create(G)
    try:
        backs = upload(q)
        ans, trd = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(tr).to("cuda:0")
        cnt = torch.zeros(counters_size(B), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        collective(L, comm, q, q.ops[0], backs)
        base = cnt.data_ptr()
        _lib.check(L.scv_aggregate_i32(L.scv_comm_ctx(comm, 2), C.c_void_p(ans.data_ptr()), None, None, C.c_void_p(trd.data_ptr()), P, B, N, _lib.MEM_DEVICE,
                                       None, None, C.c_void_p(base), C.c_void_p(base + 8 * B * _lib.TIE_CLASSES), C.c_void_p(base + 8 * (B * _lib.TIE_CLASSES + B))))
        for r in range(G):
            _lib.check(L.scv_export_error_word(L.scv_comm_ctx(comm, r), C.c_void_p(backs[r].data_ptr() + 8 * (q.off + n))))
        collective(L, comm, q, q.ops[1], backs)
        with pytest.raises(_lib.DomainError):                            # once, although ranks 0 and 1 are clean
            _lib.check(L.scv_comm_sync(comm))
        _lib.check(L.scv_comm_sync(comm))
        words = [int(b.cpu()[q.off + n]) for b in backs]
        assert words[0] != 0 and words == [words[0]] * G, words
        want = cf.model(q)
        for w in want:
            w[q.off + n] = words[0]
        assert_equal_to_model(q, backs, want)                            # the collectives around the error are exact on every rank
    finally:
        L.scv_comm_destroy(comm)


# ---- 8. C5 with degenerate shards --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [2, 5, 8])
def test_c5_on_shards_without_problems_and_without_resamples(G, engines):
    N, B, seed = 40, 2, 99
    me = engines(G)
    rng = np.random.default_rng(1000 + G)
    for P in sorted({1, G - 1, G, G + 1}):
        tables = [(rng.integers(0, 6, size=(P, B, N), dtype=np.int32), rng.integers(0, 6, size=P, dtype=np.int32))]
        if P == G - 1:
            tables.append((tables[0][0], np.full(P, 1000, dtype=np.int32)))           # the truth is nobody's answer: every cell a miss
        for a, tr in tables:
            want = coracle.aggregate(a, tr)
            M = int(want["cells"]["n_modes"][want["cells"]["hit"] == 1].max(initial=0)) + 1
            host = me.aggregate(a, tr)                                   # HOST mode over the same shards (ranks without problems take no part)
            assert np.array_equal(host.tie_class_hits, want["tie_class_hits"]) and np.array_equal(host.truth_count_sum, want["truth_count_sum"])
            for f in CELL_FIELDS:
                assert np.array_equal(host.cells[f], want["cells"][f]), (P, f)
            shards = [(s[0], s[1], None) for s in me.scatter(a, tr)]
            for R in sorted({0, 1, G - 1, G + 1}):
                rc, want_boot = coracle.bootstrap(want["cells"], 0, R, seed, M)
                assert rc == 0 and want_boot.shape == (R, B, M)
                for M_arg in (None, M):
                    _, _, _, M_got = me.evaluate_c5(shards, R, seed, M=M_arg, keep_all_ranks=True)
                    me.sync()
                    assert M_got == M, (P, R, M_arg)
                    for g in range(G):                                   # every rank's copy of the three exchanged buffers
                        where = (P, R, M_arg, g)
                        cnt = me.last_c5["counters"][g].cpu().numpy()
                        got = AggregateResult.from_counters(cnt[:-1], P, B)
                        assert np.array_equal(got.tie_class_hits, want["tie_class_hits"]), where
                        assert np.array_equal(got.truth_count_sum, want["truth_count_sum"]) and cnt[-1] == 0, where
                        cells = cells_from_torch(me.last_c5["tables"][g])
                        for f in CELL_FIELDS:
                            assert np.array_equal(cells[f], want["cells"][f]), (where, f)
                        assert np.array_equal(me.last_c5["boots"][g].cpu().numpy(), want_boot), where
