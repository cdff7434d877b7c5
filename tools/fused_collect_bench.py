#!/usr/bin/env python3
"""Rollout collection through the one-launch collect tick (TrainerConfig.fused_collect) against today's path: profiles/fused_collect.txt.

    python tools/fused_collect_bench.py [--envs 4096] [--maps squarinth labyrinth] [--horizon 128] [--reps 6] [--warmup 3]
                                        [--ratio] [--regs FILE] [--out profiles/fused_collect.txt]

1. Speed.  Per map two trainers in one process, ``fused_collect`` off (the per-layer path, unchanged: the baseline) and on, each over its own env
   from the same seeds.  After ``--warmup`` collect + update rounds of each (the eager rollout, the capture, a replay; the update's graphs), every
   repetition measures both, the order alternating from repetition to repetition (off-on, on-off, ...):
     - collection us per tick: device events around ``collect()`` (one replay of the captured rollout graph) / horizon;
     - collect + update env-steps/s: host clock around ``collect(); update()`` that ends in a device synchronise.
   Median and min .. max over the repetitions are recorded: the spread says what a difference is worth.
2. ``--ratio``: the ``ratio`` step of tests/collect_steps.py in a child process; its figure line is recorded.
3. ``--regs FILE``: a register / scratch record of csrc/cat_act.hip (-Rpass-analysis=kernel-resource-usage), copied in.
What is not asked for is recorded as "not taken"."""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def speed_section(a):
    import dataclasses
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
    rc = dataclasses.replace(CFG_AGENT, random_timesteps=0, learning_starts=0)
    out = [f"## 1. speed: {a.envs} envs, 2v1, 64 rays, {a.horizon}-tick rollouts, bptt 16; {a.warmup} warm-up rounds, {a.reps} repetitions, order alternating",
           "#    median (min .. max)"]
    fmt = lambda v, p: f"{statistics.median(v):.{p}f} ({min(v):.{p}f} .. {max(v):.{p}f})"
    for name in a.maps:
        legs = {}
        for fused in (False, True):
            env = VecCopsEnv(load_preset(name, 2, 1), a.envs, num_rays=64, max_step_count=400, seed=1)
            tcfg = TrainerConfig(horizon=a.horizon, policy_freeze_duration=0, opponent_freeze_duration=0, fused_collect=fused)
            legs[fused] = (env, MAPPOTrainer(env, {"cop": rc, "thief": rc}, tcfg, seed=0))
        for _ in range(a.warmup):
            for _, tr in legs.values():
                tr.collect(); tr.update()
        torch.cuda.synchronize()
        res = {f: {"tick_us": [], "steps_s": []} for f in legs}
        for r in range(a.reps):
            for fused in ((False, True) if r % 2 == 0 else (True, False)):
                _, tr = legs[fused]
                assert tr._graph is not None, "the rollout is not captured"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record(); tr.collect(); e1.record()
                tr.update()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res[fused]["tick_us"].append(e0.elapsed_time(e1) * 1e3 / a.horizon)
                res[fused]["steps_s"].append(a.horizon * a.envs / dt / 1e6)
        for fused, label in ((False, "fused_collect off"), (True, "fused_collect on ")):
            out.append(f"{name:10s} {label}: collection {fmt(res[fused]['tick_us'], 1)} us/tick   collect + update {fmt(res[fused]['steps_s'], 3)} M env-steps/s")
        off, on = (statistics.median(res[f]["tick_us"]) for f in (False, True))
        out.append(f"{name:10s} collection, on / off: {on / off:.3f} (medians)")
        for env, _ in legs.values():
            env.check_errors()
            env.close()
        del legs
        torch.cuda.empty_cache()
    return out


def ratio_section(a):
    out = ["", "## 2. stored log-probability against the training forward's (tests/collect_steps.py, step ratio)"]
    if not a.ratio:
        return out + ["not taken (--ratio)"]
    r = subprocess.run([sys.executable, "-m", "tests.collect_steps", "ratio"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("ratio:")]
    return out + (lines if r.returncode == 0 and lines else [f"FAILED rc={r.returncode}"] + r.stdout.splitlines()[-5:])


def regs_section(a):
    out = ["", "## 3. registers and scratch of csrc/cat_act.hip"]
    return out + (Path(a.regs).read_text().rstrip().splitlines() if a.regs else ["not taken (--regs FILE)"])


def main():
    import torch
    from bench import source_sha16
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", nargs="+", default=["squarinth", "labyrinth"])
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--regs", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fused_collect.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fused_collect_bench: no GPU; nothing is measured without one")
    lines = [f"# rollout collection: cat_act_collect_step (TrainerConfig.fused_collect) against the per-layer path; env-core source {source_sha16()}; "
             f"{torch.cuda.get_device_name(0)}"]
    lines += speed_section(a) + ratio_section(a) + regs_section(a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
