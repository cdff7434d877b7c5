"""CPU: the host-side pieces of bench.py that need no GPU (the measurement itself is covered by the -m gpu tests)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_algorithmic_bytes_follow_survey_8d():
    assert bench.algorithmic_bytes_per_env_step(3, 64) == 1292          # 108 A + 3 A R + 6 R + 8
    assert bench.algorithmic_bytes_per_env_step(5, 64) == 108 * 5 + 3 * 5 * 64 + 6 * 64 + 8


def test_short_regions_carry_no_per_dispatch_events():
    assert bench.event_stride(20) == 0      # the driver's --steps 20: one event pair around all 20 launches (timed_steps), none attached to a dispatch
    assert bench.event_stride(2000) == 8


def test_cpu_share_is_bounded_by_the_box_share():
    n = bench.host_cpu_share()
    assert 1 <= n <= 16


def test_committed_traffic_file_matches_the_headline_workload_and_says_its_regime():
    newest = sorted((ROOT / "profiles").glob("r*_traffic.json"))[-1]
    prof = json.loads(newest.read_text())
    assert prof["workload_key"] == {"map": "labyrinth", "envs": 4096, "rays": 64, "cops": 2, "thieves": 1}
    assert "running batch" in prof["regime"] and prof["burn_in"] == 600
    assert prof["hbm_bytes_per_launch"] > bench.algorithmic_bytes_per_env_step(3, 64) * 4096       # counters >= algorithmic bytes
    assert prof["hbm_bytes_per_launch_from_reset"] and prof["hbm_bytes_per_launch_from_reset"] <= prof["hbm_bytes_per_launch"]
    assert 0.3 < prof["valu"]["lane_utilisation"] < 1.0


def test_plain_multi_gpu_command_is_a_launcher_invocation(monkeypatch):
    """`python bench.py --gpus 4` without WORLD_SIZE: the parent builds a torch.distributed.run command line on 127.0.0.1 with one
    process per GPU and hands its own arguments through (the GPU test runs it; here the command is only inspected)."""
    seen = {}

    class _Done:
        returncode = 0

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return _Done()
    import subprocess
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5"])
    monkeypatch.setenv("RANK", "3")                      # stale launcher variables must not leak into the children
    assert bench.launch_ranks(4) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]
    assert "RANK" not in seen["env"] and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_arguments_a_run_cannot_honour_are_refused(monkeypatch, capsys):
    import pytest
    for argv, msg in ((["--steps", "0"], "--steps must be at least 1"), (["--shape-only"], "--shape-only restricts --full")):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        with pytest.raises(SystemExit) as exc:
            bench.main()
        assert exc.value.code == 2 and msg in capsys.readouterr().err


def test_dumped_outputs_are_float32_and_a_large_batch_keeps_the_same_seeded_rows(tmp_path, monkeypatch):
    """--dump-outputs on host tensors: every output field widened to float32 without loss; over the size limit, one seeded sample of
    env rows is taken from every array and its indices are written beside them, the same rows on every run."""
    import numpy as np
    import torch
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    N, gen = 500, torch.Generator().manual_seed(1)
    sim = type("FakeSim", (), {})()
    sim.device, sim.N = torch.device("cpu"), N
    sim.out = {"obs_distance": (torch.rand(N, 3, 8, generator=gen) * 500).half(), "obs_type": torch.randint(0, 4, (N, 3, 8), generator=gen, dtype=torch.uint8),
               "reward": torch.randn(N, 3, generator=gen), "winner": torch.randint(-1, 2, (N,), generator=gen, dtype=torch.int8)}
    bench.dump_outputs(sim, tmp_path / "all", 0, 1)
    for k, v in sim.out.items():
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.float().numpy())
    assert not (tmp_path / "all" / "env_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20_000)
    for run in ("s1", "s2"):
        bench.dump_outputs(sim, tmp_path / run, 0, 1)
    rows = np.load(tmp_path / "s1" / "env_index.npy")
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "env_index.npy")) and 0 < len(rows) < N
    assert np.all(np.diff(rows) > 0) and rows[-1] < N
    assert sum(np.load(tmp_path / "s1" / f"{k}.npy").nbytes for k in sim.out) <= 20_000
    for k, v in sim.out.items():
        assert np.array_equal(np.load(tmp_path / "s1" / f"{k}.npy"), v.float().numpy()[rows.astype(np.int64)])
