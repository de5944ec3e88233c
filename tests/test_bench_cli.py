"""bench.py's command line where no GPU is needed: the multi-GPU form of the driver's command on a box with fewer
devices than ranks (here: none) must answer with ONE JSON line carrying "error" and a non-zero exit status -- never a
traceback, never silence -- and must not need a launcher in front."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_launcher_and_without_devices_is_one_error_line():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("covered by the gpu-marked form (device count + 1 ranks)")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, cwd=REPO, env=env)
    assert out.returncode != 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout + out.stderr
    d = json.loads(lines[0])
    assert "error" in d and "--gpus 8" in d["error"] and d["n_gpus"] == 8 and d["hip_devices_visible"] == 0


def test_spawn_command_is_the_drivers_own_launcher_line(monkeypatch):
    """What bench.py runs for `python bench.py --gpus 4 --steps 2`: torch.distributed.run, one node, 4 processes,
    rendezvous on 127.0.0.1, the same script with the same arguments (the contract's launch line)."""
    import importlib
    import types
    sys.path.insert(0, REPO)
    bench = importlib.import_module("bench")
    seen = {}

    def fake_run(cmd, **kw):
        seen["cmd"], seen["env"] = cmd, kw.get("env", {})
        return types.SimpleNamespace(returncode=0, stdout='{"metric": "m", "n_gpus": 4}\n')

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2", "--share-device", "--backend", "gloo"])
    args = bench.parse()
    assert bench.spawn_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-7:] == [os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "2", "--share-device", "--backend", "gloo"][-7:]
    assert seen["env"]["SCV_BENCH_SPAWNED"] == "1"


def test_a_plain_run_leaves_every_leg_but_the_headline_to_full(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` only sets up, warms up and times: the cpu_baseline leg with its parity checks, c3_full, the
    live read ceiling and the live roofline.traffic run with --full alone, where the --no-* options still switch single legs off."""
    import importlib
    sys.path.insert(0, REPO)
    bench = importlib.import_module("bench")
    legs = lambda a: (a.no_cpu_baseline, a.full_pass, a.no_read_ceiling, a.live_traffic)  # noqa: E731
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert legs(a) == (True, False, True, False) and a.steps == 5 and a.warmup == 2 and a.dump_outputs is None
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--full"])
    assert legs(bench.parse()) == (False, True, False, True)
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--no-full-pass", "--dump-outputs", "d"])
    a = bench.parse()
    assert legs(a) == (True, False, False, True) and a.dump_outputs == "d"


def test_dump_outputs_writes_float64_arrays_and_a_fixed_sample_beyond_64_mb(tmp_path):
    import importlib

    import numpy as np
    sys.path.insert(0, REPO)
    bench = importlib.import_module("bench")
    counters = np.arange(8 * 1027, dtype=np.int64) * ((1 << 39) + 1)          # up to 2^52: exact in float64
    cells = np.zeros((3, 2), dtype=[("max_count", "<u4"), ("truth_count", "<u4"), ("n_modes", "<u2"), ("min_mode", "<i2"), ("hit", "u1")])
    cells["min_mode"] = -1
    bench.dump_outputs(str(tmp_path / "small"), dict(counters=counters, **bench.cell_fields(cells), cell_tokens=None))
    names = sorted(os.listdir(tmp_path / "small"))
    assert names == ["cells_hit.npy", "cells_max_count.npy", "cells_min_mode.npy", "cells_n_modes.npy", "cells_truth_count.npy", "counters.npy"]
    got = np.load(tmp_path / "small" / "counters.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.int64), counters)
    assert np.array_equal(np.load(tmp_path / "small" / "cells_min_mode.npy"), np.full((3, 2), -1.0))
    big = np.arange(3 << 20, dtype=np.int64).reshape(-1, 8)                  # 24 MB as float64, x 4 arrays > 64 MB
    arrays = {f"a{i}": big + i for i in range(4)}
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = sum(os.path.getsize(tmp_path / "x" / n) for n in os.listdir(tmp_path / "x"))
    assert total <= 64 << 20
    rows = np.load(tmp_path / "x" / "a2_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "x" / "a2.npy"), (big + 2)[rows]) and np.all(np.diff(rows) > 0)
    for n in os.listdir(tmp_path / "x"):
        assert np.array_equal(np.load(tmp_path / "x" / n), np.load(tmp_path / "y" / n)), n
