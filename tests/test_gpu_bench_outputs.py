"""GPU: a plain bench.py run is the headline alone, and --dump-outputs writes what its last timed step handed the caller.  The dumped
arrays are held against the CPU oracle stepped through the same ticks (reset, burn-in, warm-up, timed steps; Philox actions of each
tick, auto-reset of the envs that ended), bit for bit."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
OUT_KEYS = ("obs_distance", "obs_type", "shared_distance", "shared_type", "team_positions", "reward", "terminated", "truncated", "winner")


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    envs, burn_in, warmup, steps = 64, 390, 5, 45          # 440 ticks: the 400-tick timeouts land in the warm-up
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--envs", str(envs), "--burn-in", str(burn_in),
                          "--warmup", str(warmup), "--steps", str(steps), "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] == pytest.approx(envs * steps / (d["ms_per_step"] * 1e-3 * steps), rel=1e-9)
    assert d["device_errors"] == 0 and d["roofline"]["kernel_ms"] > 0
    assert "extra" not in d and "cpu_baseline" not in d and "traffic" not in d["roofline"]     # --full only

    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert sorted(got) == sorted(OUT_KEYS)
    assert all(a.dtype == np.float32 and a.shape[0] == envs for a in got.values())

    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.maps import load_preset
    from oracle.cat_oracle import OracleSim
    cfg = SimConfig(n_envs=envs, n_cops=2, n_thieves=1, n_rays=64, max_step_count=400, seed=0, env_id_offset=0)   # bench.build_sim's
    cpu = OracleSim(cfg, [load_preset("labyrinth", 2, 1).compile()])
    cpu.reset()
    for t in range(burn_in + warmup + steps):
        c = cpu.step(cpu.random_actions(t))
        flags = {k: c[k].copy() for k in ("reward", "terminated", "truncated", "winner")}
        cpu.reset(mask=c["terminated"].copy())
    widen = lambda a: (a.view(np.float16) if a.dtype == np.uint16 else a).astype(np.float32)   # the oracle keeps float16 as raw bits
    want = {k: widen(np.asarray(v)) for k, v in cpu.out.items() if k in OUT_KEYS}
    want.update({k: widen(v) for k, v in flags.items()})
    for k in OUT_KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
