"""The guard-band draws of tests/_agg_guard.py on the CPU: what they reach (asked of csrc/scvote_plan.h through tests/plan_check.cpp), that the
checker catches every fault it is there for (planted by a numpy stand-in for the engine that writes into a host copy of the arena), and that the
expected results -- which come from oracle.coracle alone -- agree with oracle/pyoracle.py on a handful of draws."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from oracle import pyoracle
from tests import _agg_guard as G

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed in range(G.DEFAULT_SEEDS):
        c = G.draw(seed)
        regions, size = G.layout(c)
        arena = G.host_arena(c, regions, size)
        res = G.oracle_outputs(c)
        out.append((c, regions, arena, G.expected_arena(c, regions, arena, res), res))
    return out


@pytest.fixture(scope="module")
def reached(cases, tmp_path_factory):
    """seed -> the kernel family the plan gives the draw."""
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "plan_check.cpp")])
    ask = lambda lines: subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()  # noqa: E731
    first = ask([line for c, *_ in cases for line in G.plan_queries(c)])
    assert len(first) == 8 * len(cases)
    per = [first[8 * i:8 * i + 8] for i in range(len(cases))]
    second = []
    for (c, *_), ans in zip(cases, per):
        opts = [line for line in G.plan_queries(c) if line.startswith(("reset", "opt"))]
        lane_fits = int(ans[7].split()[0])
        second += opts + [f"form {c.B} {c.N} {int(G.rows_aligned(c))} {lane_fits} {int(ans[6])}"]
    forms = ask(second)
    assert len(forms) == len(cases)
    return {c.seed: G.plan_of(c, ans, form) for (c, *_), ans, form in zip(cases, per, forms)}


# the kernels every default run must reach, each at least three times: every Kind (LANE through its four kernels, SORT, REG through every forced
# shape, STREAM whole / split-N / with the reduce launch), every PrefixForm and both sort-prefix kernels
REQUIRED = (["scv_one_vote", "scv_two_votes", "scv_few_votes", "scv_lane_cells", "scv_sort_cells", "stream", "stream_split", "stream_reduce"] +
            [f"reg_{code}" for code in (*G.SPARSE_SHAPES, *G.DENSE_SHAPES)] + ["reg_803", "reg_804"] +
            ["scv_sort_prefix", "scv_sort_prefix2", "prefix_POOL", "prefix_CELLS", "prefix_LANE", "prefix_HIST"])


def _group(label):
    return "REG" if label.startswith("reg_") else ("STREAM" if label.startswith("stream") else ("PREFIX" if "prefix" in label else
                                                                                                   ("SORT" if label == "scv_sort_cells" else "LANE")))


def test_the_default_seeds_reach_every_kernel_and_every_output_form(cases, reached):
    counts = Counter(reached.values())
    print(sorted(counts.items()))
    assert not [k for k in REQUIRED if counts[k] < 3], sorted(counts.items())
    # within each kind: cells / no cells, overwrite / accumulate, tokens / none -- and packed / 16-byte records where packed records are served
    forms = {}
    for c, *_ in cases:
        f = forms.setdefault(_group(reached[c.seed]), Counter())
        f["cells" if c.want_cells else "no_cells"] += 1
        f["overwrite" if c.overwrite else "accumulate"] += 1
        f["tokens" if c.tokens_on else "no_tokens"] += 1
        f["ctok_pointer_without_tokens"] += int(c.ctok_given and not c.tokens_on)
        if c.want_cells:
            f["packed" if c.packed else "wide"] += 1
    print({k: dict(v) for k, v in forms.items()})
    for kind in ("LANE", "SORT", "REG", "STREAM", "PREFIX"):
        for form in ("cells", "no_cells", "overwrite", "accumulate", "tokens", "no_tokens", "ctok_pointer_without_tokens", "wide"):
            assert forms[kind][form] >= 3, (kind, form, dict(forms[kind]))
    for kind in ("LANE", "SORT", "REG"):
        assert forms[kind]["packed"] >= 3, (kind, dict(forms[kind]))
    assert forms["STREAM"]["packed"] == 0 and forms["PREFIX"]["packed"] == 0          # never drawn where the library refuses them
    # the alignment classes: votes over all four, the cell tables and the counters at odd multiples of their requirement on about half the draws
    assert {c.align["votes"] for c, *_ in cases} == {0, 4, 8, 12} and {c.align["tokens"] for c, *_ in cases} == {0, 4, 8, 12}
    for name, odd in (("cells", 16), ("cell_tokens", 16), ("counters", 8)):
        n = sum(c.align[name] == odd for c, *_ in cases)
        assert len(cases) // 3 <= n <= 2 * len(cases) // 3, (name, n)
    for c, regions, *_ in cases:
        ends = sorted((o, o + n) for o, n in regions.values())
        assert ends[0][0] >= G.GUARD and all(b[0] - a[1] >= G.GUARD for a, b in zip(ends, ends[1:]))
        for name, align in (("cells", G.CELL_ALIGN), ("cell_tokens", G.CTOK_ALIGN), ("counters", G.COUNTER_ALIGN)):
            assert regions[name][0] % align == 0 and regions[name][0] % 32 == c.align[name]
    # the ragged budgets hold every edge
    seen = set()
    for c, *_ in cases:
        if c.n_valid is not None:
            seen |= {("0", "1", "N-1", "N", "N+1")[i] for i, v in enumerate((0, 1, c.N - 1, c.N, c.N + 1)) if v in c.n_valid.tolist()}
    assert seen == {"0", "1", "N-1", "N", "N+1"}


# ---- the checker catches what it is for ---------------------------------------------------------------------------------------------------------

def _stand_in(c, regions, arena, res, fault=None):
    """What a correct engine leaves in the arena -- or one with a fault planted.  Returns (arena, error word)."""
    got = G.expected_arena(c, regions, arena, res)
    rec = 4 if c.packed else 16
    o, n = regions["cells"]
    err = 0
    if fault == "past":
        got[o + n:o + n + rec] = 0x11
    elif fault == "before":
        got[o - rec:o] = 0x11
    elif fault == "wide_record":                     # a 16-byte record for the last cell of a packed table
        got[o + n - 4:o + n - 4 + 16] = np.frombuffer(res["cells"].reshape(-1)[-1:].tobytes(), dtype=np.uint8)
    elif fault == "ctok_without_tokens":
        o2, n2 = regions["cell_tokens"]
        got[o2:o2 + n2] = 0
    elif fault == "cells_unasked":
        got[o:o + n] = np.frombuffer(res["cells"].tobytes(), dtype=np.uint8)
    elif fault == "counters_early":
        o3, n3 = regions["counters"]
        got[o3 - 8:o3 - 8 + n3] = got[o3:o3 + n3].copy()
    elif fault == "input_changed":
        o4, n4 = regions["votes"]
        got[o4 + (c.seed * 4) % n4] ^= 1
    elif fault == "guard_vote":                      # the word behind the last row is counted as a vote: it is outside the domain
        assert np.all(arena[regions["votes"][0] + regions["votes"][1]:][:4] == G.INPUT_GUARD)
        err = 1
    return got, err


FAULTS = {"past": lambda c: c.want_cells, "before": lambda c: c.want_cells, "wide_record": lambda c: c.want_cells and c.packed,
          "ctok_without_tokens": lambda c: not c.tokens_on, "cells_unasked": lambda c: not c.want_cells, "counters_early": lambda c: True,
          "input_changed": lambda c: c.votes.size > 0, "guard_vote": lambda c: True}


def test_the_checker_passes_a_correct_engine_and_flags_every_planted_fault(cases):
    applies, caught = Counter(), Counter()
    for c, regions, arena, want, res in cases:
        got, err = _stand_in(c, regions, arena, res)
        G.check(c, regions, want, got, err)
        for fault, applicable in FAULTS.items():
            if not applicable(c):
                continue
            applies[fault] += 1
            got, err = _stand_in(c, regions, arena, res, fault)
            try:
                G.check(c, regions, want, got, err)
            except AssertionError as e:
                caught[fault] += 1
                assert c.stratum in str(e)
    print(dict(applies))
    for fault in FAULTS:
        assert applies[fault] >= 20 and caught[fault] == applies[fault], (fault, applies[fault], caught[fault])      # 100 % of the draws it applies to


def test_the_message_names_the_table_and_the_offset(cases):
    c, regions, arena, want, res = next(x for x in cases if x[0].want_cells)
    got, _ = _stand_in(c, regions, arena, res, "past")
    with pytest.raises(AssertionError, match="0 bytes behind the end of cells"):
        G.check(c, regions, want, got)
    got, _ = _stand_in(c, regions, arena, res, "counters_early")
    with pytest.raises(AssertionError, match="8 bytes before counters"):
        G.check(c, regions, want, got)


# ---- the oracle anchor ----------------------------------------------------------------------------------------------------------------------------

def test_a_handful_of_draws_agree_with_the_python_oracle(cases):
    pinned = 0
    for c, _, _, _, res in cases:
        if c.P * c.B * max(c.N, 1) > 40_000 or pinned >= 12 or c.seed % 5:
            continue
        pinned += 1
        for p in range(c.P):
            for b in range(c.B):
                n = c.N if c.n_valid is None else int(np.clip(c.n_valid[b], 0, c.N))
                row = (c.votes[p] if c.prefix else c.votes[p, b])[:n].tolist()
                ref = pyoracle.cell_integers(row, int(c.truth[p]))
                cell = res["cells"][p, b]
                assert (int(cell["max_count"]), int(cell["truth_count"]), int(cell["n_modes"]), int(cell["hit"])) == \
                       (ref["max_count"], ref["truth_count"], ref["n_modes"], ref["hit"]), (c.seed, p, b)
                assert int(cell["min_mode"]) == (min(ref["modes"]) if ref["modes"] else -1)
                if c.tokens_on:
                    trow = (c.tokens[p] if c.prefix else c.tokens[p, b])[:n]
                    assert int(res["cell_tokens"][p, b]) == int(trow.astype(np.int64).sum())
    assert pinned >= 5
