"""The communicator draws of tests/_comm_fuzz.py, without a GPU: the numpy model equals a word-by-word Python statement of the three
collectives on the cheap draws; the default seeds reach every stratum the draws are weighted for, by exact conditions; and six wrong
collectives differ from the model on a stated share of the default draws, so a communicator with one of those mistakes cannot pass
tests/test_gpu_comm_fuzz.py."""
import numpy as np
import pytest

from tests import _comm_fuzz as cf

SEEDS = range(cf.DEFAULT_SEEDS)
CHEAP_DIV = 100                                                          # the anchor's draws: <= 4 * 10^4 words * ranks per sequence
VARIANTS = ("last_rank_left_out", "stops_at_16384", "whole_blocks_only", "block_at_rank_times_max", "write_ignored", "rank0_only")
COLLECTIVES = ("allreduce", "allgather_i64", "allgather_cells")


@pytest.fixture(scope="module")
def cases():
    """The default draws with the model's final arrays: computed once, left unchanged."""
    out = []
    for s in SEEDS:
        q = cf.draw(s)
        q.want = cf.model(q)
        for w in q.want:
            w.setflags(write=False)
        out.append(q)
    return out


def naive(q):
    """The three collectives and the write, word by word, in Python ints reduced mod 2^64."""
    M = 1 << 64
    bufs = [[int(x) % M for x in back[q.off:q.off + q.W]] for back in q.init]
    for op in q.ops:
        if op[0] == "allreduce":
            for i in range(op[1]):
                s = 0
                for r in range(q.G):
                    s = (s + bufs[r][i]) % M
                for r in range(q.G):
                    bufs[r][i] = s
        elif op[0] in ("allgather_i64", "allgather_cells"):
            words = [c if op[0] == "allgather_i64" else c * op[2] * 2 for c in op[1]]
            start = 0
            for j in range(q.G):
                for i in range(start, start + words[j]):
                    for r in range(q.G):
                        bufs[r][i] = bufs[j][i]
                start += words[j]
        elif op[0] == "write":
            _, r, a, b = op
            for i in range(q.W):
                bufs[r][i] = (bufs[r][i] * a + b) % M
    out = []
    for back, buf in zip(q.init, bufs):
        full = [int(x) for x in back]
        full[q.off:q.off + q.W] = [x - M if x >= M // 2 else x for x in buf]
        out.append(np.array(full, dtype=np.int64))
    return out


def test_draws_depend_on_the_seed_alone():
    for s in (0, 7, 59):
        a, b = cf.draw(s), cf.draw(s)
        assert cf.describe(a) == cf.describe(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a.init, b.init))
    assert cf.describe(cf.draw(3)) != cf.describe(cf.draw(4))


def test_every_draw_is_a_valid_sequence_inside_the_work_bound(cases):
    for q in cases:
        d = cf.describe(q)
        assert q.G in cf.G_CHOICES and q.off in (3, 4) and len(q.init) == q.G and 1 <= len(q.ops) <= 12, d
        assert all(x.dtype == np.int64 and x.shape == (q.off + q.W + cf.GUARD,) for x in q.init), d
        work = 0
        for op in q.ops:
            assert op[0] in cf.OP_KINDS, d
            if op[0] in COLLECTIVES:
                assert 0 <= cf.extent(op) <= q.W and all(c >= 0 for c in (op[1] if op[0] != "allreduce" else [op[1]])), d
                assert op[0] == "allreduce" or len(op[1]) == q.G, d
                work += cf.extent(op) * q.G
            elif op[0] == "write":
                assert 0 <= op[1] < q.G and -2 ** 63 <= op[2] < 2 ** 63 and -2 ** 63 <= op[3] < 2 ** 63, d
                work += q.W
        assert work == q.work <= cf.WORK, d
        assert sum(1 for op in q.ops if op[0] == "allreduce" and op[1] > cf.STAGING_WORDS) <= 2, d
        assert sum(1 for op in q.ops if op[0] in COLLECTIVES) >= 1, d


def test_the_model_equals_the_word_by_word_statement_on_the_cheap_draws():
    seen = set()
    for s in range(40):
        q = cf.draw(s, work_div=CHEAP_DIV)
        assert q.work <= cf.WORK // CHEAP_DIV, cf.describe(q)
        got, want = cf.model(q), naive(q)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), cf.describe(q)
        seen |= {op[0] for op in q.ops}
        for g, back in zip(got, q.init):                                # the guards are the drawn ones
            assert np.array_equal(g[:q.off], back[:q.off]) and np.array_equal(g[q.off + q.W:], back[q.off + q.W:])
    assert seen == set(cf.OP_KINDS)


def test_the_default_seeds_reach_every_stratum(cases):
    def some(pred, at_least=1):
        n = sum(1 for q in cases if pred(q))
        assert n >= at_least, n
        return n

    def colls(q):
        return [op for op in q.ops if op[0] in COLLECTIVES]

    def ar_counts(q):
        return [op[1] for op in q.ops if op[0] == "allreduce"]

    for G in cf.G_CHOICES:
        some(lambda q: q.G == G, 5)
    for count in cf.AR_EDGES:                                            # 0, 16384 / 16385 (the grid-stride loop), 131072 / 131073 (the staging buffer) among them
        some(lambda q: count in ar_counts(q) and q.G > 1, 2)
    some(lambda q: any(c > cf.AR_EDGES[-1] for c in ar_counts(q)))       # a random count above every edge
    some(lambda q: any(c % 256 and c > 256 for c in ar_counts(q)), 10)

    def collective_behind_a_growth(q):
        ops = colls(q)
        return any(op[0] == "allreduce" and op[1] > cf.STAGING_WORDS and i + 1 < len(ops) for i, op in enumerate(ops)) and q.G > 1
    some(collective_behind_a_growth, 3)

    def a_sum_wraps(q):
        """An all-reduce whose exact integer sum of some word leaves int64 (replayed through the model op by op)."""
        backs = [np.array(x) for x in q.init]
        bufs = [b[q.off:q.off + q.W].view(np.uint64) for b in backs]
        for op in q.ops:
            if op[0] == "allreduce" and op[1] and q.G > 1:
                exact = np.sum(np.stack([b[:op[1]].view(np.int64).astype(object) for b in bufs]), axis=0)
                if any(not -2 ** 63 <= int(x) < 2 ** 63 for x in exact[:64]):
                    return True
            cf.apply(q, bufs, op)
        return False
    some(a_sum_wraps, 10)

    gathers = lambda q: [op for op in q.ops if op[0] in ("allgather_i64", "allgather_cells")]       # noqa: E731
    ragged = lambda op: sum(op[1]) > 0                                                               # noqa: E731
    some(lambda q: q.G >= 3 and any(ragged(op) and op[1][0] == 0 for op in gathers(q)), 2)
    some(lambda q: q.G >= 3 and any(ragged(op) and op[1][q.G // 2] == 0 for op in gathers(q)), 2)
    some(lambda q: q.G >= 3 and any(ragged(op) and op[1][-1] == 0 for op in gathers(q)), 2)
    some(lambda q: any(not ragged(op) for op in gathers(q)), 3)                                      # an all-zero gather
    some(lambda q: q.G > 1 and any(sorted(op[1])[-2] == 0 and ragged(op) for op in gathers(q)), 3)  # one rank owns everything
    some(lambda q: q.G > 1 and any(set(op[1]) == {1} for op in gathers(q) if op[0] == "allgather_i64"))       # blocks of one word
    some(lambda q: q.G > 1 and any(set(op[1]) == {1} and op[2] == 1 for op in gathers(q) if op[0] == "allgather_cells"))   # ... of one cell
    for B in cf.CELL_B:
        some(lambda q: any(op[0] == "allgather_cells" and op[2] == B for op in q.ops))
    some(lambda q: q.G > 1 and any(max(op[1]) * (1 if op[0] == "allgather_i64" else 2 * op[2]) > cf.STAGING_WORDS for op in gathers(q)), 2)   # a block above 1 MiB
    for off in (3, 4):                                                   # 24 bytes (8-byte aligned only) and 32 bytes into the allocation
        some(lambda q: q.off == off, 15)
    for vk in cf.VALUE_KINDS:
        some(lambda q: q.value_kind == vk, 3)

    def write_between_two_collectives(q):
        kinds = [op[0] for op in q.ops if op[0] != "rebind"]
        return any(k == "write" and set(kinds[:i]) & set(COLLECTIVES) and set(kinds[i + 1:]) & set(COLLECTIVES) for i, k in enumerate(kinds))
    some(write_between_two_collectives, 20)
    some(lambda q: any(a[0] in COLLECTIVES and b[0] in COLLECTIVES for a, b in zip(q.ops, q.ops[1:])), 20)    # two collectives back to back
    some(lambda q: ("rebind",) in q.ops, 15)


def share(cases, variant):
    n = 0
    for q in cases:
        got = cf.model(q, variant)
        n += any(not np.array_equal(g, w) for g, w in zip(got, q.want))
    return n / len(cases)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_collective_differs_on_a_tenth_of_the_default_draws(cases, variant):
    """The project's bar for fuzz sensitivity.  Measured on the 60 default draws: DESIGN.md §6."""
    s = share(cases, variant)
    print(f"{variant}: {100 * s:.0f} % of {len(cases)} draws differ")
    assert s >= 0.10, (variant, s)


def test_the_variants_leave_the_guards_alone(cases):
    """A variant differs inside the working buffers only: what the GPU test adds by comparing the guards is not measured here."""
    for q in cases[:12]:
        for v in VARIANTS:
            for g, back in zip(cf.model(q, v), q.init):
                assert np.array_equal(g[:q.off], back[:q.off]) and np.array_equal(g[q.off + q.W:], back[q.off + q.W:])
